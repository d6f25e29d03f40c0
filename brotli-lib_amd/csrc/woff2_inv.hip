// Inverse WOFF2 'glyf' / 'hmtx' transforms on the GPU (W3C WOFF2 sections 5.1 - 5.4): the
// transformed tables that mib_decode gets out of a .woff2 become the TrueType glyf, loca and
// hmtx tables again, byte for byte as fontTools 4.62 reconstructs and compiles them.
//
// Unlike the forward pass (woff2.hip), where loca says where each glyph's bytes are, here a
// glyph's position in six variable-length streams has to be found first (DESIGN.md,
// "WOFF2 inverse"):
//   inv_count_kernel    per glyph: contours, bbox bit, composite -> scanned
//   inv_npoints_kernel  one wave: the 255UInt16 boundaries of the nPoints stream, up to 64
//                       speculated (one byte each) per step -> points per contour -> scanned
//   inv_comp_kernel     one wave: each composite's length and haveInstructions; the lanes
//                       digest the stream into LDS, a wave-uniform walk follows the components
//   inv_measure_kernel  per glyph: its flag offset, triplet bytes T[g], other cursors
//   inv_chain_kernel    one wave: off[g+1] = off[g] + T[g] + len255(stream[off[g] + T[g]]),
//                       64 glyphs per step speculated with len255 = 1
//   inv_size_kernel     per glyph: the shared walker (woff2_inv.h) sizes the record and
//                       checks that it stops where the next glyph's cursors start
//   inv_write_kernel    per glyph: the walker again, writing;  inv_loca_kernel: loca
// The parsing itself is woff2_inv.h, which the CPU tests run under sanitizers.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "common.h"
#include "woff2_dev.h"
#include "woff2_inv.h"

namespace mib {
namespace woff2inv {

constexpr int kWave = 64;
enum { kCntContours, kCntBBox, kCntComp, kCounts };

// the per-glyph cursor arrays, each num_glyphs + 1 long ([num_glyphs]: where the stream ends)
struct CurArrays {
  uint32_t *c[kStreams];
};

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x, int lane) {
  for (int d = 1; d < kWave; d <<= 1) {
    const uint32_t y = __shfl_up(x, d, kWave);
    if (lane >= d) x += y;
  }
  return x;
}

// counts[k][ng + 1]: glyph g's contours, bbox bit, composite flag; [ng] = 0 so that the
// exclusive scan's entry ng is the total
__global__ void inv_count_kernel(View v, uint32_t *counts, int *bad) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t ng = v.num_glyphs;
  if (g > ng) return;
  uint32_t nc = 0, bb = 0, co = 0;
  if (g < ng) {
    const int32_t c = ncontours(v, g);
    if (c < -1) atomicOr(bad, 1);
    nc = c > 0 ? (uint32_t)c : 0;
    co = c == -1;
    bb = c != 0 && bit_of(v.bbox_bm, g);
  }
  counts[(size_t)kCntContours * (ng + 1) + g] = nc;
  counts[(size_t)kCntBBox * (ng + 1) + g] = bb;
  counts[(size_t)kCntComp * (ng + 1) + g] = co;
}

// One wave.  pts[c], pos[c] for contour c < cap (cap = bytes in the stream: a contour takes
// at least one); pos[C] = where the stream's values end.  Zeroed beforehand.
__global__ void inv_npoints_kernel(View v, const uint32_t *xcont /* scanned */, uint32_t *pts, uint32_t *pos,
                                   uint32_t *steps, int *bad) {
  const int lane = threadIdx.x;
  const uint32_t ng = v.num_glyphs, n = v.n[kNPoints];
  uint32_t C = xcont[ng] - xcont[0];
  if (C > n) {   // more contours than bytes
    if (lane == 0) atomicOr(bad, 1);
    C = n;
  }
  uint32_t base = 0, c = 0, nsteps = 0;
  while (c < C) {
    nsteps++;
    const uint32_t p = base + lane;
    const bool in_c = c + lane < C, in_s = p < n;
    const uint32_t b = (in_c && in_s) ? v.s[kNPoints][p] : 0;
    const unsigned long long stop = __ballot(!in_c || !in_s || len255_code(b) != 1);
    const int m = stop ? __ffsll(stop) - 1 : kWave;
    if (lane < m) {
      pts[c + lane] = b;
      pos[c + lane] = p;
    }
    if (m == kWave) {
      base += kWave;
      c += kWave;
      continue;
    }
    const int m_in_c = __shfl((int)in_c, m, kWave), m_in_s = __shfl((int)in_s, m, kWave);
    c += m;
    base += m;
    if (!m_in_c) break;   // every contour placed
    if (!m_in_s) {        // the stream ends before the contours do
      if (lane == 0) atomicOr(bad, 1);
      break;
    }
    // lane m is a boundary too (everything before it took one byte): a longer value
    uint32_t q = p;
    int bd = 0;
    const uint32_t val = rd255(v, kNPoints, q, bd);
    if (lane == m) {
      pts[c] = val;
      pos[c] = p;
      if (bd) atomicOr(bad, 1);
    }
    base = __shfl(q, m, kWave);
    c += 1;
    if (__shfl(bd, m, kWave)) break;
  }
  if (lane == 0) {
    pos[c] = base;
    steps[0] = nsteps;
  }
}

// One wave.  Composite k < cap: coff[k] = its offset in the composite stream, chi[k] = whether
// it has instructions; coff[ncomp] = the end.  The stream goes through LDS a window at a time
// (all lanes load and pre-digest it), lane 0 walks the components in it.
constexpr uint32_t kCompWindow = 8192;
__global__ void inv_comp_kernel(View v, const uint32_t *xcomp /* scanned */, uint32_t cap, uint32_t *coff,
                                uint32_t *chi, int *bad) {
  __shared__ uint8_t win[kCompWindow / 2];   // one code per even offset of the window
  const int lane = threadIdx.x;
  const uint32_t ng = v.num_glyphs, n = v.n[kComposite];
  uint32_t ncomp = __builtin_amdgcn_readfirstlane(xcomp[ng] - xcomp[0]);
  if (ncomp > cap) {
    if (lane == 0) atomicOr(bad, 1);
    ncomp = cap;
  }
  // The walk is the same in every lane (what it reads from LDS goes through readfirstlane), so
  // its state stays in scalar registers and its branches are scalar: a one-lane walk under an
  // exec mask measured several times slower.  Every lane stores the same words.
  uint32_t pos = 0, k = 0;
  bool fail = false;
  while (k < ncomp && !fail) {
    // window [w0, w0 + wn): the walk stops when a component's flags (2 bytes) would leave it
    const uint32_t w0 = pos, wn = n - w0 < kCompWindow ? n - w0 : kCompWindow;
    // Component lengths are even, so a component of this window starts at an even offset: the
    // lanes turn the flag word at every even offset into one byte (length / 2, MORE_COMPONENTS,
    // WE_HAVE_INSTRUCTIONS), and the dependent chain is one LDS byte a component.
    __syncthreads();
    for (uint32_t i = lane; 2 * i + 2 <= wn; i += kWave) {
      const uint32_t fl = ((uint32_t)v.s[kComposite][w0 + 2 * i] << 8) | v.s[kComposite][w0 + 2 * i + 1];
      win[i] = (uint8_t)((comp_len(fl) >> 1) | ((fl & kMore) ? 16 : 0) | ((fl & kHaveInstr) ? 32 : 0));
    }
    __syncthreads();
    bool open = false, hi = false;   // inside a composite (its MORE_COMPONENTS chain)
    uint32_t start = pos;            // ... which began here
    for (;;) {
      if (!open) {
        if (k >= ncomp) break;
        coff[k] = pos;
        start = pos;
        hi = false;
        open = true;
      }
      if (pos + 2 > n) {   // a component was promised and the stream is over
        fail = true;
        break;
      }
      if (pos + 2 > w0 + wn) break;   // next window
      const uint32_t code = __builtin_amdgcn_readfirstlane(win[(pos - w0) >> 1]);
      const uint32_t next = pos + 2 * (code & 15);
      if (next > n) {
        fail = true;
        break;
      }
      pos = next;
      hi = hi || (code & 32);
      if (!(code & 16)) {
        chi[k] = hi;
        k++;
        open = false;
      }
    }
    // a composite cut by the window's end starts over in the next window, from its own start
    if (open && !fail) {
      pos = start;
      if (pos == w0) {   // it does not fit a window: walk it from memory
        int bd = 0;
        bool h2;
        comp_walk(v, pos, h2, bd);
        pos = __builtin_amdgcn_readfirstlane(pos);
        if (__builtin_amdgcn_readfirstlane(bd)) fail = true;
        else {
          chi[k] = h2;
          k++;
        }
      }
    }
  }
  if (lane == 0) {
    if (fail) atomicOr(bad, 1);
    else coff[k] = pos;
  }
}

// Per glyph (and one thread for the end entry): the cursors that need no chain, the glyph's
// triplet bytes T and whether a 255UInt16 instruction length follows them.
__global__ void inv_measure_kernel(View v, const uint32_t *counts_x, const uint32_t *pts_x, const uint32_t *pos,
                                   const uint32_t *coff, const uint32_t *chi, uint32_t comp_cap, CurArrays cur,
                                   uint32_t *T, uint32_t *has255) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t ng = v.num_glyphs;
  if (g > ng) return;
  const uint32_t *xc = counts_x + (size_t)kCntContours * (ng + 1), *xb = counts_x + (size_t)kCntBBox * (ng + 1),
                 *xk = counts_x + (size_t)kCntComp * (ng + 1);
  const uint32_t cap = v.n[kNPoints];
  uint32_t c0 = xc[g] - xc[0], c1 = (g < ng ? xc[g + 1] : xc[g]) - xc[0];
  c0 = c0 < cap ? c0 : cap;
  c1 = c1 < cap ? c1 : cap;
  uint32_t k = xk[g] - xk[0];
  k = k < comp_cap ? k : comp_cap;
  const uint32_t fl0 = pts_x[c0], npts = pts_x[c1] - fl0;
  cur.c[kNPoints][g] = pos[c0];
  cur.c[kFlags][g] = fl0;
  cur.c[kComposite][g] = coff[k];
  cur.c[kBBox][g] = 8 * (xb[g] - xb[0]);
  uint32_t t = 0, h = 0;
  if (g < ng) {
    const int32_t nc = ncontours(v, g);
    if (nc > 0) {
      h = 1;
      const uint32_t nf = v.n[kFlags];
      if (fl0 <= nf && npts <= nf - fl0 && npts <= 65536)   // (else the sizing pass rejects the glyph)
        for (uint32_t i = 0; i < npts; i++) t += (uint32_t)trip_len(v.s[kFlags][fl0 + i]);
    } else if (nc == -1) {
      h = chi[k] != 0;
    }
  }
  T[g] = t;
  has255[g] = h;
}

// One wave.  gl[g] = glyph g's offset in the glyph stream, ilen[g] = its instruction length
// (0 without one), gl[ng] = the end.  Each step speculates that the next 64 glyphs' lengths
// take one byte each, accepts all before the first that does not, and resumes after it: an
// unhinted font moves 64 glyphs a step, a fully hinted one at least one.
__global__ void inv_chain_kernel(View v, const uint32_t *T, const uint32_t *has255, uint32_t *gl, uint32_t *ilen,
                                 uint32_t *steps, int *bad) {
  const int lane = threadIdx.x;
  const uint32_t ng = v.num_glyphs, n = v.n[kGlyph];
  uint32_t base = 0, g0 = 0, nsteps = 0;
  int fail = 0;
  while (g0 < ng) {
    nsteps++;
    const uint32_t g = g0 + lane;
    const bool in_g = g < ng;
    const uint32_t t = in_g ? T[g] : 0, h = in_g ? has255[g] : 0;
    const uint32_t incl = wave_incl_scan(t + h, lane), excl = incl - (t + h);
    const uint32_t p = base + excl + t;   // (64 glyphs of at most 4 * 65536 + 1 bytes: no wrap)
    const bool in_s = p < n;
    const uint32_t b = (h && in_s) ? v.s[kGlyph][p] : 0;
    const unsigned long long stop = __ballot(!in_g || (h && (!in_s || len255_code(b) != 1)));
    const int m = stop ? __ffsll(stop) - 1 : kWave;
    if (lane < m) {
      gl[g] = base + excl;
      ilen[g] = h ? b : 0;
    }
    if (m == kWave) {
      base += __shfl(incl, kWave - 1, kWave);
      g0 += kWave;
    } else {
      const int m_in_g = __shfl((int)in_g, m, kWave);
      const uint32_t m_start = base + __shfl(excl, m, kWave);
      g0 += m;
      if (!m_in_g) {   // past the last glyph
        base = m_start;
        break;
      }
      uint32_t q = p;
      int bd = 0;
      const uint32_t val = rd255(v, kGlyph, q, bd);   // (lane m: h is set, p is its length's place)
      if (lane == m) {
        gl[g] = m_start;
        ilen[g] = val;
      }
      base = __shfl(q, m, kWave);
      g0 += 1;
      fail = __shfl(bd, m, kWave);
    }
    if (base > n) fail = 1;
    if (fail) break;
  }
  if (lane == 0) {
    if (fail) atomicOr(bad, 1);
    gl[ng] = base > n ? n : base;
    ilen[ng] = 0;
    steps[1] = nsteps;
  }
}

__device__ __forceinline__ Cursors cursors_of(const CurArrays &cur, uint32_t g) {
  Cursors k;
  k.c[kNContour] = 0;
  for (int s = kNPoints; s < kStreams; s++) k.c[s] = cur.c[s][g];
  return k;
}

// sizes[g] = glyph g's padded record (0 for a rejected one), sizes[ng] = 0
__global__ void inv_size_kernel(View v, CurArrays cur, uint32_t *sizes, int *bad) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g > v.num_glyphs) return;
  uint32_t sz = 0;
  if (g < v.num_glyphs) {
    const Cursors k = cursors_of(cur, g), next = cursors_of(cur, g + 1);
    Cursors end;
    bool ok = walk_glyph(v, g, k, nullptr, &sz, &end);
    // the resolution passes and the walker must agree on where the glyph's bytes end
    for (int s = kNPoints; s < kStreams; s++) ok = ok && end.c[s] == next.c[s];
    if (!ok) {
      atomicOr(bad, 1);
      sz = 0;
    }
  }
  sizes[g] = sz;
}

__global__ void inv_write_kernel(View v, CurArrays cur, const uint32_t *off, uint8_t *out) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= v.num_glyphs || off[g + 1] == off[g]) return;
  uint32_t sz;
  Cursors end;
  walk_glyph(v, g, cursors_of(cur, g), out + off[g], &sz, &end);
}

__global__ void inv_loca_kernel(uint32_t ng, uint32_t long_loca, const uint32_t *off, uint8_t *loca) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= ng) put_loca(loca, long_loca, i, off[i]);
}

// blockIdx.y (and on by gridDim.y): the font; blockIdx.x: its glyphs.  (n >= 1: the table's flags
// are its first byte)
__global__ void inv_hmtx_kernel(const mib::woff2dev::HmtxFont *fonts, uint32_t k, int *bad) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  for (uint32_t f = blockIdx.y; f < k; f += gridDim.y) {
    const mib::woff2dev::HmtxFont d = fonts[f];
    if (g >= d.ng) continue;
    if (!hmtx_flags_ok(d.t[0], d.n, d.ng, d.nhm)) {   // nothing behind the flags is read then
      atomicOr(bad + f, 1);
      continue;
    }
    if (!hmtx_glyph(d.t, d.glyf, d.glyf_n, d.loca, d.long_loca, d.ng, d.nhm, g, d.out)) atomicOr(bad + f, 1);
  }
}

}  // namespace woff2inv
}  // namespace mib

using namespace mib::woff2inv;
using mib::woff2dev::Call;
using mib::woff2dev::DevMem;
using mib::woff2dev::HmtxFont;
using mib::woff2dev::Timer;

namespace {

bool scan(DevMem &m, const uint32_t *in, uint32_t *out, size_t count, hipStream_t st) {
  size_t tmp_b = 0;
  if (hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_b, in, out, (int)count, st) != hipSuccess) return false;
  uint8_t *tmp = m.take<uint8_t>(tmp_b);
  return tmp && hipcub::DeviceScan::ExclusiveSum(tmp, tmp_b, in, out, (int)count, st) == hipSuccess;
}

uint32_t g_last_steps[2];   // the last call's speculation steps (nPoints chain, glyph-stream chain)

}  // namespace

// diagnostic (DESIGN.md's measurements): the speculation steps of the last reconstruct_glyf
extern "C" void mib_woff2_inv_last_steps(uint32_t out[2]) {
  out[0] = g_last_steps[0];
  out[1] = g_last_steps[1];
}

int mib::woff2dev::reconstruct_glyf_device(hipStream_t st, Timer &tm, DevMem &m, DevMem &keep, const uint8_t *hdr,
                                           const uint8_t *d_t, size_t n, uint8_t **d_glyf, size_t *glyf_b_out,
                                           uint8_t **d_loca, size_t *loca_b_out) {
  View hv, v;
  if (!parse_header(hdr, n, hdr, &hv) || !parse_header(hdr, n, d_t, &v)) return MIB_E_INVALID_ARG;
  const uint32_t ng = hv.num_glyphs;
  const size_t g1 = (size_t)ng + 1;
  const uint32_t np_cap = hv.n[kNPoints], comp_cap = hv.n[kComposite] / 6 + 1;
  uint32_t *d_counts = m.take<uint32_t>(kCounts * g1), *d_counts_x = m.take<uint32_t>(kCounts * g1);
  uint32_t *d_pts = m.take<uint32_t>((size_t)np_cap + 1), *d_pts_x = m.take<uint32_t>((size_t)np_cap + 1);
  uint32_t *d_pos = m.take<uint32_t>((size_t)np_cap + 1);
  uint32_t *d_coff = m.take<uint32_t>((size_t)comp_cap + 1), *d_chi = m.take<uint32_t>((size_t)comp_cap + 1);
  uint32_t *d_cur = m.take<uint32_t>(kStreams * g1);
  uint32_t *d_T = m.take<uint32_t>(g1), *d_h = m.take<uint32_t>(g1), *d_ilen = m.take<uint32_t>(g1);
  uint32_t *d_sizes = m.take<uint32_t>(g1), *d_off = m.take<uint32_t>(g1);
  uint32_t *d_steps = m.take<uint32_t>(2);
  int *d_bad = m.take<int>(1);
  if (!d_counts || !d_counts_x || !d_pts || !d_pts_x || !d_pos || !d_coff || !d_chi || !d_cur || !d_T || !d_h || !d_ilen ||
      !d_sizes || !d_off || !d_steps || !d_bad)
    return MIB_E_OUT_OF_MEMORY;
  CurArrays cur;
  for (int s = 0; s < kStreams; s++) cur.c[s] = d_cur + (size_t)s * g1;
  hipMemsetAsync(d_bad, 0, 4, st);
  hipMemsetAsync(d_steps, 0, 8, st);
  hipMemsetAsync(d_pts, 0, 4 * ((size_t)np_cap + 1), st);
  hipMemsetAsync(d_pos, 0, 4 * ((size_t)np_cap + 1), st);
  hipMemsetAsync(d_coff, 0, 4 * ((size_t)comp_cap + 1), st);
  hipMemsetAsync(d_chi, 0, 4 * ((size_t)comp_cap + 1), st);
  hipMemsetAsync(d_cur, 0, 4 * kStreams * g1, st);
  hipMemsetAsync(d_ilen, 0, 4 * g1, st);
  const dim3 grid1((uint32_t)((g1 + 255) / 256)), block(256);
  bool ok = true;
  tm.start("w2inv_count");
  hipLaunchKernelGGL(inv_count_kernel, grid1, block, 0, st, v, d_counts, d_bad);
  tm.stop();
  tm.start("w2inv_scan_counts");
  ok = ok && scan(m, d_counts, d_counts_x, kCounts * g1, st);
  tm.stop();
  tm.start("w2inv_npoints");
  hipLaunchKernelGGL(inv_npoints_kernel, dim3(1), dim3(kWave), 0, st, v, d_counts_x + (size_t)kCntContours * g1, d_pts,
                     d_pos, d_steps, d_bad);
  tm.stop();
  tm.start("w2inv_scan_points");
  ok = ok && scan(m, d_pts, d_pts_x, (size_t)np_cap + 1, st);
  tm.stop();
  tm.start("w2inv_comp");
  hipLaunchKernelGGL(inv_comp_kernel, dim3(1), dim3(kWave), 0, st, v, d_counts_x + (size_t)kCntComp * g1, comp_cap, d_coff,
                     d_chi, d_bad);
  tm.stop();
  tm.start("w2inv_measure");
  hipLaunchKernelGGL(inv_measure_kernel, grid1, block, 0, st, v, d_counts_x, d_pts_x, d_pos, d_coff, d_chi, comp_cap, cur,
                     d_T, d_h);
  tm.stop();
  tm.start("w2inv_chain");
  hipLaunchKernelGGL(inv_chain_kernel, dim3(1), dim3(kWave), 0, st, v, d_T, d_h, cur.c[kGlyph], d_ilen, d_steps, d_bad);
  tm.stop();
  tm.start("w2inv_scan_instr");
  ok = ok && scan(m, d_ilen, cur.c[kInstr], g1, st);
  tm.stop();
  tm.start("w2inv_size");
  hipLaunchKernelGGL(inv_size_kernel, grid1, block, 0, st, v, cur, d_sizes, d_bad);
  tm.stop();
  tm.start("w2inv_scan_sizes");
  ok = ok && scan(m, d_sizes, d_off, g1, st);
  tm.stop();
  if (!ok) {
    hipStreamSynchronize(st);
    return MIB_E_OUT_OF_MEMORY;
  }
  int bad = 0;
  uint32_t total = 0, steps[2] = {0, 0};
  Cursors end;
  end.c[kNContour] = 0;
  hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, st);
  hipMemcpyAsync(&total, d_off + ng, 4, hipMemcpyDeviceToHost, st);
  hipMemcpyAsync(steps, d_steps, 8, hipMemcpyDeviceToHost, st);
  for (int s = kNPoints; s < kStreams; s++) hipMemcpyAsync(&end.c[s], cur.c[s] + ng, 4, hipMemcpyDeviceToHost, st);
  if (hipStreamSynchronize(st) != hipSuccess) return MIB_E_NO_DEVICE;
  g_last_steps[0] = steps[0];
  g_last_steps[1] = steps[1];
  // a malformed glyph; streams not used up exactly; offsets that loca format 0 cannot hold
  if (bad || !totals_ok(hv, end, total)) return MIB_E_INVALID_ARG;
  // the size comes from the sizing pass alone (every glyph empty: one zero byte, as fontTools)
  const size_t glyf_b = total ? total : 1, loca_b = g1 * (hv.long_loca ? 4 : 2);
  uint8_t *d_out = keep.take<uint8_t>(glyf_b + loca_b);
  if (!d_out) return MIB_E_OUT_OF_MEMORY;
  if (!total) hipMemsetAsync(d_out, 0, 1, st);
  tm.start("w2inv_write");
  hipLaunchKernelGGL(inv_write_kernel, grid1, block, 0, st, v, cur, d_off, d_out);
  tm.stop();
  tm.start("w2inv_loca");
  hipLaunchKernelGGL(inv_loca_kernel, grid1, block, 0, st, ng, hv.long_loca, d_off, d_out + glyf_b);
  tm.stop();
  *d_glyf = d_out;
  *glyf_b_out = glyf_b;
  *d_loca = d_out + glyf_b;
  *loca_b_out = loca_b;
  return 0;
}

extern "C" int mib_woff2_reconstruct_glyf(const uint8_t *tglyf, size_t n, mib_buf *glyf, mib_buf *loca) {
  if (!glyf || !loca) return MIB_E_INVALID_ARG;
  glyf->data = loca->data = nullptr;
  glyf->size = loca->size = 0;
  if (!tglyf) return MIB_E_INVALID_ARG;
  View hv;
  if (!parse_header(tglyf, n, tglyf, &hv)) return MIB_E_INVALID_ARG;
  Call use(true);
  if (!use.c) return MIB_E_NO_DEVICE;
  uint8_t *d_t = use.m.take<uint8_t>(n), *d_glyf = nullptr, *d_loca = nullptr;
  size_t glyf_b = 0, loca_b = 0;
  if (!d_t) return use.rc = MIB_E_OUT_OF_MEMORY;
  hipMemcpyAsync(d_t, tglyf, n, hipMemcpyHostToDevice, use.st);
  if ((use.rc = mib::woff2dev::reconstruct_glyf_device(use.st, use.tm, use.m, use.m, tglyf, d_t, n, &d_glyf, &glyf_b, &d_loca,
                                                       &loca_b)))
    return use.rc;
  // two results, one synchronisation (Call::fetch would take one each)
  glyf->data = mib_buf_alloc(glyf_b);
  loca->data = mib_buf_alloc(loca_b);
  if (glyf->data && loca->data) {
    glyf->size = glyf_b;
    loca->size = loca_b;
    hipMemcpyAsync(glyf->data, d_glyf, glyf_b, hipMemcpyDeviceToHost, use.st);
    hipMemcpyAsync(loca->data, d_loca, loca_b, hipMemcpyDeviceToHost, use.st);
    use.rc = hipStreamSynchronize(use.st) == hipSuccess ? 0 : MIB_E_NO_DEVICE;
  } else {
    use.rc = MIB_E_OUT_OF_MEMORY;
  }
  if (use.rc) {
    mib::woff2dev::drop(glyf);
    mib::woff2dev::drop(loca);
  }
  use.timed = use.rc == 0;
  return use.rc;
}

void mib::woff2dev::launch_hmtx(hipStream_t st, Timer &tm, const HmtxFont *d_fonts, size_t k, uint32_t most_ng, int *d_bad) {
  const uint32_t rows = (uint32_t)(k < 65535 ? k : 65535);   // (the kernel walks on by gridDim.y)
  tm.start("w2inv_hmtx");
  hipLaunchKernelGGL(inv_hmtx_kernel, dim3((most_ng + 255) / 256, rows), dim3(256), 0, st, d_fonts, (uint32_t)k, d_bad);
  tm.stop();
}

// The launch over one font: the table's flags and size are checked on the device, as in the file
// decoder's launch over many (woff2_file.hip).
extern "C" int mib_woff2_reconstruct_hmtx(const uint8_t *thmtx, size_t n, const uint8_t *glyf, size_t glyf_n,
                                          const uint8_t *loca, size_t loca_n, uint32_t num_glyphs,
                                          uint32_t num_hmetrics, mib_buf *out) {
  if (!out) return MIB_E_INVALID_ARG;
  out->data = nullptr;
  out->size = 0;
  uint32_t long_loca = 0;
  if (!loca || (!glyf && glyf_n) ||
      !hmtx_args_ok(thmtx, n, glyf_n, loca_n, num_glyphs, num_hmetrics, &long_loca))
    return MIB_E_INVALID_ARG;
  Call use(true);
  if (!use.c) return MIB_E_NO_DEVICE;
  const size_t total = 4 * (size_t)num_hmetrics + 2 * (size_t)(num_glyphs - num_hmetrics);
  uint8_t *d_in = use.m.take<uint8_t>(n + glyf_n + loca_n), *d_out = use.m.take<uint8_t>(total);
  int *d_bad = use.m.take<int>(1);
  HmtxFont *d_font = use.m.take<HmtxFont>(1);
  if (!d_in || !d_out || !d_bad || !d_font) return use.rc = MIB_E_OUT_OF_MEMORY;
  hipMemcpyAsync(d_in, thmtx, n, hipMemcpyHostToDevice, use.st);
  if (glyf_n) hipMemcpyAsync(d_in + n, glyf, glyf_n, hipMemcpyHostToDevice, use.st);
  hipMemcpyAsync(d_in + n + glyf_n, loca, loca_n, hipMemcpyHostToDevice, use.st);
  const HmtxFont font{d_in, (uint64_t)n, d_in + n, d_in + n + glyf_n, d_out, (uint32_t)glyf_n, long_loca, num_glyphs, num_hmetrics};
  hipMemsetAsync(d_bad, 0, 4, use.st);
  hipMemcpyAsync(d_font, &font, sizeof(font), hipMemcpyHostToDevice, use.st);   // (synchronised below)
  mib::woff2dev::launch_hmtx(use.st, use.tm, d_font, 1, num_glyphs, d_bad);
  int bad = 0;
  hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, use.st);
  if (hipStreamSynchronize(use.st) != hipSuccess) return use.rc = MIB_E_NO_DEVICE;
  // flags that do not fit the size; a loca entry that does not fit the glyf table
  if (bad) {
    use.timed = true;   // (the kernel ran)
    return use.rc = MIB_E_INVALID_ARG;
  }
  use.rc = use.fetch(d_out, total, out);
  use.timed = use.rc == 0;
  return use.rc;
}
