// An sfnt -> the .woff2 file that stands for it (DESIGN.md 4c "Writing a file").  The container is
// planned on the host (woff2_write.h); on the device the fonts of a group are uploaded once, glyf
// and hmtx are transformed from them in place (woff2.hip's cores), every other table is copied to
// its place in the font's stream by one launch of
//   w2enc_pack_kernel   every untransformed table of every font (blockIdx.x: the table, its 4 KiB
//                       tiles over blockIdx.y): copied over the destination's 16-byte granules,
//                       head's checkSumAdjustment cleared and its flags bit 11 set on the way
// and one encode call (FONT mode) on the default context compresses all streams.  Only the
// transforms' sizes and flags visit the host between the upload and the download of the compressed
// streams, each of which lands directly behind the header and directory the host wrote into the
// result.  mib_woff2_encode is the batch with k = 1.
// An OpenType collection (woff2_write_ttc.h, DESIGN.md 4c "Writing a collection") is one file and
// one stream of its group.  Which of its tables are one by content is decided, for all collections
// of the group at once and before anything is sized, by one launch of
//   w2enc_same_kernel   every candidate (blockIdx.x: a record and its representative, both of any
//                       alignment; 4 KiB tiles over blockIdx.y): compared exactly, 16 bytes a
//                       thread; a difference stores 1 into the candidate's flag
// whose flags the host reads after one synchronisation.  A collection without candidates, and a
// call of single fonts only, launch nothing of it.
#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "common.h"
#include "load16.h"
#include "woff2_batch.h"
#include "woff2_dev.h"
#include "woff2_write.h"
#include "woff2_write_ttc.h"

namespace mib {
namespace woff2write {

constexpr uint32_t kPackThreads = 256;
constexpr uint64_t kPackTile = (uint64_t)kPackThreads * 16;   // bytes of the stream a block covers at a time
constexpr uint32_t kPackSpread = 256;                         // blocks per table at most (each walks its tiles)
constexpr uint64_t kEncSlack = 512;   // zero bytes behind the last stream (the encoder's kernels read past a stream's end)

// One untransformed table.  src has any alignment and 16 readable bytes of slack behind its
// allocation's last byte (load16.h); dst is its place in the launch's stream buffer, whose base is
// a multiple of 16.
struct PackDesc {
  const uint8_t *src;
  uint64_t dst;
  uint32_t len;
  uint32_t head;   // HeadFix
};

// Tiles are laid over the destination's 16-byte granules, from the table's place in the stream
// buffer: a granule whose 16 bytes are all the table's moves as one vector, its unaligned source
// read through load16_any; the head and tail granules move byte by byte, so neighbouring tables
// (the streams have no padding) never touch each other's bytes.  The granules that hold head's
// bytes 8..16 take the byte path too, where 8..11 are stored as zero and bit 3 of byte 16 is set.
__global__ __launch_bounds__(kPackThreads) void w2enc_pack_kernel(const PackDesc *descs, uint8_t *out) {
  const PackDesc d = descs[blockIdx.x];
  const uint32_t mis = (uint32_t)(d.dst & 15);
  const uint64_t tiles = d.len ? ((uint64_t)d.len + mis + kPackTile - 1) / kPackTile : 0;
  uint8_t *dst = out + d.dst;
  for (uint64_t t = blockIdx.y; t < tiles; t += gridDim.y) {
    const int64_t lo = (int64_t)(16 * (t * kPackThreads + threadIdx.x)) - (int64_t)mis;   // the granule's first byte in the table
    if (lo >= (int64_t)d.len) continue;
    if (lo >= 0 && (uint64_t)lo + 16 <= d.len && !(d.head != kHeadNone && lo <= 16)) {
      *reinterpret_cast<uint4 *>(dst + lo) = load16_any(d.src + lo);
    } else {
#pragma unroll
      for (int q = 0; q < 16; q++) {
        const int64_t at = lo + q;
        if (at < 0 || at >= (int64_t)d.len) continue;   // another table's byte
        uint32_t b = d.src[at];
        if (d.head != kHeadNone && at >= 8 && at < 12) b = 0;
        if (d.head == kHeadZeroFlag && at == 16) b |= 0x08;
        dst[at] = (uint8_t)b;
      }
    }
  }
}

// One candidate: two ranges of len bytes, each of any alignment and with 16 readable bytes of slack
// behind its allocation's last byte.
struct SameDesc {
  const uint8_t *a, *b;
  uint32_t len;
};

// Tiles are laid over the ranges from their first bytes: a granule whose 16 bytes all belong to the
// ranges is read as one vector from each side (load16_any), the last partial granule byte by byte.
// differ[] is zeroed in front of the launch; a block that has stored skips its remaining tiles.
__global__ __launch_bounds__(kPackThreads) void w2enc_same_kernel(const SameDesc *descs, uint8_t *differ) {
  const SameDesc d = descs[blockIdx.x];
  const uint64_t tiles = ((uint64_t)d.len + kPackTile - 1) / kPackTile;
  for (uint64_t t = blockIdx.y; t < tiles; t += gridDim.y) {   // (uniform over the block: the barrier below)
    const uint64_t lo = 16 * (t * kPackThreads + threadIdx.x);
    bool diff = false;
    if (lo + 16 <= d.len) {
      const uint4 x = load16_any(d.a + lo), y = load16_any(d.b + lo);
      diff = x.x != y.x || x.y != y.y || x.z != y.z || x.w != y.w;
    } else {
      for (uint64_t at = lo; at < d.len; at++) diff |= d.a[at] != d.b[at];
    }
    if (diff) differ[blockIdx.x] = 1;
    if (__syncthreads_or(diff)) break;
  }
}

}  // namespace woff2write
}  // namespace mib

using namespace mib::woff2write;
using mib::woff2dev::Call;
using mib::woff2dev::DevMem;
using mib::woff2dev::drop;
using mib::woff2dev::GlyfIn;
using mib::woff2dev::GlyfSized;
using mib::woff2dev::HmtxSized;
using mib::woff2dev::Timer;

extern "C" uint64_t mib_encode_out_bound(uint64_t n);

namespace {

struct GroupFont {   // a font or a collection of the group whose plan parsed
  size_t slot;       // in the call's arrays
  Plan *pl;          // a single font's plan, or
  TtcPlan *tp;       // a collection's
  const uint8_t *d_font;
  GlyfSized gz;      // a single font's
  HmtxSized hz;
  std::vector<GlyfSized> gzs;   // a collection's: per pair, per hmtx unit
  std::vector<HmtxSized> hzs;
  bool alive;
  uint64_t stream_at;   // its stream in the group's stream buffer
};

// The compare launch alone: differ[i] = 1 where descs[i]'s ranges differ.  Synchronises the stream.
int same_device(hipStream_t st, Timer &tm, DevMem &m, const std::vector<SameDesc> &descs, uint8_t *differ) {
  const size_t k = descs.size();
  if (k > 0x7FFFFFFFull) return MIB_E_INVALID_ARG;
  SameDesc *d_descs = m.take<SameDesc>(k);
  uint8_t *d_differ = m.take<uint8_t>(k);
  if (!d_descs || !d_differ) return MIB_E_OUT_OF_MEMORY;
  uint64_t most_tiles = 1;
  for (const SameDesc &d : descs) most_tiles = std::max(most_tiles, ((uint64_t)d.len + kPackTile - 1) / kPackTile);
  if (hipMemsetAsync(d_differ, 0, k, st) != hipSuccess ||
      hipMemcpyAsync(d_descs, descs.data(), sizeof(SameDesc) * k, hipMemcpyHostToDevice, st) != hipSuccess)
    return MIB_E_NO_DEVICE;
  const uint32_t spread = (uint32_t)(most_tiles < kPackSpread ? most_tiles : kPackSpread);
  tm.start("w2enc_same");
  hipLaunchKernelGGL(w2enc_same_kernel, dim3((uint32_t)k, spread), dim3(kPackThreads), 0, st, d_descs, d_differ);
  tm.stop();
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(differ, d_differ, k, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return MIB_E_NO_DEVICE;
  return 0;
}

// The transforms' sizes of one collection, pair after pair and hmtx unit after hmtx unit, and its
// layout.  MIB_E_INVALID_ARG: this collection's affair.
int size_collection(hipStream_t st, Timer &tm, DevMem &gm, GroupFont &f) {
  TtcPlan &tp = *f.tp;
  f.gzs.resize(tp.tr_glyf ? tp.pairs.size() : 0);
  f.hzs.resize(tp.hunits.size());
  std::vector<uint64_t> glen(f.gzs.size()), hlen(f.hzs.size());
  for (size_t p = 0; p < f.gzs.size(); p++) {
    const Table &g = tp.t[tp.pairs[p].glyf], &l = tp.t[tp.pairs[p].glyf + 1];
    const GlyfIn in{f.d_font + g.src_off, g.src_len, f.d_font + l.src_off, tp.pairs[p].num_glyphs, tp.pairs[p].long_loca};
    if (int r = mib::woff2dev::transform_glyf_size(st, tm, gm, in, &f.gzs[p])) return r;
    glen[p] = f.gzs[p].total;
  }
  for (size_t u = 0; u < f.hzs.size(); u++) {
    const TtcHmtx &hu = tp.hunits[u];
    if (int r = mib::woff2dev::transform_hmtx_size(st, tm, gm, f.gzs[hu.pair].in, f.d_font + tp.t[hu.hmtx].src_off, hu.nhm,
                                                   &f.hzs[u]))
      return r;
    hlen[u] = f.hzs[u].total;
  }
  return ttc_layout(&tp, glen.data(), hlen.data()) ? 0 : MIB_E_INVALID_ARG;
}

// One group: fonts idx[0..n) of the call, all parsed.  Non-zero: the call fails.
int encode_group(mib_ctx *c, hipStream_t st, const mib_span *sfnts, std::vector<Plan> &plans, std::vector<TtcPlan> &ttcs,
                 const std::vector<uint32_t> &ttc_of, const size_t *idx, size_t n, const mib_enc_opts &eo, uint32_t transforms,
                 mib_buf *woff2, int *status) {
  // every font from a 16-byte boundary of one upload buffer, staged on the host
  std::vector<uint64_t> base(n);
  uint64_t up_bytes = 0;
  for (size_t i = 0; i < n; i++) {
    base[i] = up_bytes = (up_bytes + 15) & ~15ull;
    up_bytes += sfnts[idx[i]].size;
  }
  std::vector<uint8_t> stage((size_t)up_bytes);
  for (size_t i = 0; i < n; i++) memcpy(stage.data() + base[i], sfnts[idx[i]].data, sfnts[idx[i]].size);
  // what the launches and copies read from the host until the stream is synchronised
  std::vector<GroupFont> fonts(n);
  std::vector<PackDesc> descs;
  std::vector<SameDesc> same;
  std::vector<uint64_t> in_off, out_off;
  int rc = 0;
  bool timed = false;
  DevMem gm;
  Timer tm{c, st, mib_ctx_profiling(c) == 1, {}};
  do {
    uint8_t *d_fonts = gm.take<uint8_t>((size_t)up_bytes);
    if (!d_fonts) {
      rc = MIB_E_OUT_OF_MEMORY;
      break;
    }
    if (hipMemcpyAsync(d_fonts, stage.data(), (size_t)up_bytes, hipMemcpyHostToDevice, st) != hipSuccess) {
      rc = MIB_E_NO_DEVICE;
      break;
    }
    for (size_t i = 0; i < n; i++) {
      GroupFont &f = fonts[i];
      f.slot = idx[i];
      f.pl = &plans[idx[i]];
      f.tp = ttc_of[idx[i]] == kNoTable ? nullptr : &ttcs[ttc_of[idx[i]]];
      f.d_font = d_fonts + base[i];
      f.alive = true;
      f.gz.total = f.hz.total = 0;
      if (f.tp)
        for (const TtcCandidate &q : f.tp->cand)
          same.push_back(SameDesc{f.d_font + f.tp->rec[q.rec].off, f.d_font + f.tp->rec[q.rep].off, f.tp->rec[q.rec].len});
    }
    // the collections' candidates, all in one launch; then their entries
    if (!same.empty()) {
      std::vector<uint8_t> differ(same.size());
      if ((rc = same_device(st, tm, gm, same, differ.data()))) break;
      size_t at = 0;
      for (GroupFont &f : fonts) {
        if (!f.tp || f.tp->cand.empty()) continue;
        if (ttc_entries(f.tp, sfnts[f.slot].data, sfnts[f.slot].size, transforms, differ.data() + at) != kOk) {
          status[f.slot] = MIB_E_INVALID_ARG;
          f.alive = false;
        }
        at += f.tp->cand.size();
      }
    }
    // the transforms' sizes, font after font, then each font's layout
    uint64_t stream_bytes = 0, bound = 0;
    for (size_t i = 0; i < n && !rc; i++) {
      GroupFont &f = fonts[i];
      if (!f.alive) continue;
      if (f.tp) {
        const int r = size_collection(st, tm, gm, f);
        if (r == MIB_E_INVALID_ARG) {   // a malformed glyph, or a stream past the limits: this collection's affair
          status[f.slot] = r;
          f.alive = false;
          continue;
        }
        if (r) {
          rc = r;
          break;
        }
        f.stream_at = stream_bytes;
        in_off.push_back(stream_bytes);
        stream_bytes += f.tp->stream_len;
        bound += mib_encode_out_bound(f.tp->stream_len);
        continue;
      }
      const Plan &pl = *f.pl;
      if (pl.tr_glyf) {
        const GlyfIn in{f.d_font + pl.t[pl.glyf].src_off, pl.t[pl.glyf].src_len, f.d_font + pl.t[pl.loca].src_off, pl.num_glyphs,
                        pl.long_loca};
        int r = mib::woff2dev::transform_glyf_size(st, tm, gm, in, &f.gz);
        if (!r && pl.hmtx_wanted)
          r = mib::woff2dev::transform_hmtx_size(st, tm, gm, in, f.d_font + pl.t[pl.hmtx].src_off, pl.num_hmetrics, &f.hz);
        if (r == MIB_E_INVALID_ARG) {   // a malformed glyph: this font's affair
          status[f.slot] = r;
          f.alive = false;
          continue;
        }
        if (r) {
          rc = r;
          break;
        }
      }
      if (!layout(f.pl, f.gz.total, f.hz.total)) {
        status[f.slot] = MIB_E_INVALID_ARG;
        f.alive = false;
        continue;
      }
      f.stream_at = stream_bytes;
      in_off.push_back(stream_bytes);
      stream_bytes += pl.stream_len;
      bound += mib_encode_out_bound(pl.stream_len);
    }
    if (rc) break;
    if (in_off.empty()) {
      timed = true;
      break;
    }
    in_off.push_back(stream_bytes);
    // the streams back to back (the encoder takes each one's exact length from the offsets)
    uint8_t *d_streams = gm.take<uint8_t>((size_t)(stream_bytes + kEncSlack)), *d_comp = gm.take<uint8_t>((size_t)(bound + 64));
    if (!d_streams || !d_comp) {
      rc = MIB_E_OUT_OF_MEMORY;
      break;
    }
    hipMemsetAsync(d_streams + stream_bytes, 0, kEncSlack, st);
    uint64_t most_tiles = 1;
    for (const GroupFont &f : fonts) {
      if (!f.alive) continue;
      const std::vector<Table> &t = f.tp ? f.tp->t : f.pl->t;
      const uint32_t fix = f.tp ? (uint32_t)kHeadNone : head_fix(*f.pl);
      for (uint32_t i = 0; i < t.size(); i++) {
        if (t[i].state != kPlain || !t[i].len) continue;
        const uint32_t head = f.tp ? f.tp->fix[i] : i == f.pl->head ? fix : (uint32_t)kHeadNone;
        descs.push_back(PackDesc{f.d_font + t[i].src_off, f.stream_at + t[i].at, t[i].len, head});
        const uint64_t tiles = ((uint64_t)t[i].len + 15 + kPackTile - 1) / kPackTile;
        most_tiles = tiles > most_tiles ? tiles : most_tiles;
      }
    }
    if (descs.size() > 0x7FFFFFFFull) {
      rc = MIB_E_INVALID_ARG;
      break;
    }
    if (!descs.empty()) {
      PackDesc *d_descs = gm.take<PackDesc>(descs.size());
      if (!d_descs) {
        rc = MIB_E_OUT_OF_MEMORY;
        break;
      }
      if (hipMemcpyAsync(d_descs, descs.data(), sizeof(PackDesc) * descs.size(), hipMemcpyHostToDevice, st) != hipSuccess) {
        rc = MIB_E_NO_DEVICE;
        break;
      }
      const uint32_t spread = (uint32_t)(most_tiles < kPackSpread ? most_tiles : kPackSpread);
      tm.start("w2enc_pack");
      hipLaunchKernelGGL(w2enc_pack_kernel, dim3((uint32_t)descs.size(), spread), dim3(kPackThreads), 0, st, d_descs, d_streams);
      tm.stop();
    }
    for (const GroupFont &f : fonts) {
      if (!f.alive) continue;
      if (f.tp) {
        const TtcPlan &tp = *f.tp;
        for (size_t p = 0; p < f.gzs.size(); p++)
          mib::woff2dev::transform_glyf_write(st, tm, f.gzs[p], d_streams + f.stream_at + tp.t[tp.pairs[p].glyf].at);
        for (size_t u = 0; u < f.hzs.size(); u++)
          if (tp.t[tp.hunits[u].hmtx].state == kTrHmtx)
            mib::woff2dev::transform_hmtx_write(st, tm, f.hzs[u], d_streams + f.stream_at + tp.t[tp.hunits[u].hmtx].at);
        continue;
      }
      const Plan &pl = *f.pl;
      if (pl.tr_glyf) mib::woff2dev::transform_glyf_write(st, tm, f.gz, d_streams + f.stream_at + pl.t[pl.glyf].at);
      if (pl.tr_hmtx) mib::woff2dev::transform_hmtx_write(st, tm, f.hz, d_streams + f.stream_at + pl.t[pl.hmtx].at);
    }
    if (hipGetLastError() != hipSuccess) {
      rc = MIB_E_NO_DEVICE;
      break;
    }
    const size_t ns = in_off.size() - 1;
    out_off.assign(ns + 1, 0);
    // (the lock is recursive: the encode runs on this context inside it, and starts the context's
    // kernel times afresh; this call's own are added behind them)
    rc = mib_ctx_encode(c, &eo, d_streams, in_off.data(), ns, d_comp, bound + 64, out_off.data(), st);
    if (rc == MIB_E_NEED_SPACE) rc = MIB_E_OUT_OF_MEMORY;   // (cannot be: `bound` is the encoder's own)
    if (rc) break;
    size_t q = 0;
    for (GroupFont &f : fonts) {
      if (!f.alive) continue;
      const uint64_t comp = out_off[q + 1] - out_off[q];
      const uint8_t *d_src = d_comp + out_off[q];
      q++;
      uint8_t hdr[mib::woff2file::kHeaderBytes];
      if (!(f.tp ? ttc_finish(*f.tp, sfnts[f.slot].data, comp, hdr) : finish(*f.pl, sfnts[f.slot].data, comp, hdr))) {
        status[f.slot] = MIB_E_INVALID_ARG;
        continue;
      }
      mib_buf *b = &woff2[f.slot];
      const std::vector<uint8_t> &dir = f.tp ? f.tp->dir : f.pl->dir;   // (a collection's: its CollectionHeader included)
      const size_t total = (size_t)(f.tp ? ttc_file_bytes(*f.tp, comp) : file_bytes(*f.pl, comp)), dir_b = dir.size();
      b->data = mib_buf_alloc(total);
      if (!b->data) {
        status[f.slot] = MIB_E_OUT_OF_MEMORY;
        continue;
      }
      b->size = total;
      memcpy(b->data, hdr, sizeof(hdr));
      memcpy(b->data + sizeof(hdr), dir.data(), dir_b);
      for (size_t at = sizeof(hdr) + dir_b + (size_t)comp; at < total; at++) b->data[at] = 0;   // the padding to 4 bytes
      if (comp) hipMemcpyAsync(b->data + sizeof(hdr) + dir_b, d_src, (size_t)comp, hipMemcpyDeviceToHost, st);
    }
    if (hipStreamSynchronize(st) != hipSuccess) {
      rc = MIB_E_NO_DEVICE;
      break;
    }
    timed = true;
  } while (0);
  if (rc) hipStreamSynchronize(st);   // nothing of this group is in flight when its buffers go
  tm.collect(timed);
  return rc;
}

int encode_batch(const mib_span *sfnts, size_t k, const mib_woff2_enc_opts *o, mib_buf *woff2, int *status) {
  mib_enc_opts eo;
  mib_enc_opts_default(&eo);
  uint32_t transforms = MIB_WOFF2_GLYF | MIB_WOFF2_HMTX;
  if (o) {
    eo.quality = o->quality;   // (clamped by the encoder, as mib_enc_opts')
    eo.lgwin = o->lgwin;
    transforms = o->transforms;
  } else {
    eo.quality = 11;
    eo.lgwin = 22;
  }
  eo.mode = MIB_MODE_FONT;
  if (transforms & ~(uint32_t)(MIB_WOFF2_GLYF | MIB_WOFF2_HMTX)) return MIB_E_INVALID_ARG;
  std::vector<Plan> plans(k);
  std::vector<TtcPlan> ttcs;
  std::vector<uint32_t> ttc_of(k, kNoTable);   // per slot: its collection plan
  std::vector<size_t> parsed;   // (before anything is allocated on the device)
  std::vector<uint64_t> lens;
  for (size_t i = 0; i < k; i++) {
    const uint8_t *p = sfnts[i].data;
    if (sfnts[i].size >= 12 && p[0] == 't' && p[1] == 't' && p[2] == 'c' && p[3] == 'f') {   // an OpenType collection
      ttcs.emplace_back();
      TtcPlan &tp = ttcs.back();
      // the entries: all there is to them where nothing is to be compared, and where something is,
      // the fewest there can be (every candidate equal) for item 19
      const bool ok = ttc_read(p, sfnts[i].size, transforms, &tp) == kOk && ttc_entries(&tp, p, sfnts[i].size, transforms, nullptr) == kOk;
      status[i] = ok ? 0 : MIB_E_INVALID_ARG;
      if (ok) ttc_of[i] = (uint32_t)(ttcs.size() - 1);
      else ttcs.pop_back();
    } else {
      status[i] = parse(p, sfnts[i].size, transforms, &plans[i]) == kOk ? 0 : MIB_E_INVALID_ARG;
    }
    if (status[i]) continue;
    parsed.push_back(i);
    lens.push_back(sfnts[i].size);
  }
  if (parsed.empty()) return 0;
  Call use(false);   // (every group has its own timer and buffers)
  if (!use.c) return MIB_E_NO_DEVICE;
  for (const mib::woff2file::Group &g : mib::woff2file::make_groups(lens, mib::woff2file::forced_group_bytes()))
    if ((use.rc = encode_group(use.c, use.st, sfnts, plans, ttcs, ttc_of, &parsed[g.first], g.count, eo, transforms, woff2, status)))
      break;
  return use.rc;
}

}  // namespace

extern "C" int mib_debug_tables_equal(const mib_span *a, const mib_span *b, const uint8_t *misalign_a, const uint8_t *misalign_b,
                                      size_t k, uint8_t *differ) {
  if (k == 0) return 0;
  if (!a || !b || !differ || k > 0x7FFFFFFFull) return MIB_E_INVALID_ARG;
  // every range at its misalignment from a 16-byte boundary of one upload buffer
  std::vector<uint64_t> at_a(k), at_b(k);
  uint64_t up = 0;
  for (size_t i = 0; i < k; i++) {
    if (a[i].size != b[i].size || a[i].size > 0xFFFFFFFFull || (!a[i].data && a[i].size) || (!b[i].data && b[i].size) ||
        (misalign_a && misalign_a[i] > 15) || (misalign_b && misalign_b[i] > 15))
      return MIB_E_INVALID_ARG;
    at_a[i] = ((up + 15) & ~15ull) + (misalign_a ? misalign_a[i] : 0);
    at_b[i] = ((at_a[i] + a[i].size + 15) & ~15ull) + (misalign_b ? misalign_b[i] : 0);
    up = at_b[i] + b[i].size;
  }
  std::vector<uint8_t> stage((size_t)up, 0xEE);
  for (size_t i = 0; i < k; i++) {
    if (a[i].size) memcpy(stage.data() + at_a[i], a[i].data, a[i].size);
    if (b[i].size) memcpy(stage.data() + at_b[i], b[i].data, b[i].size);
  }
  Call use(true);
  if (!use.c) return MIB_E_NO_DEVICE;
  uint8_t *d = use.m.take<uint8_t>((size_t)up);
  if (!d) return use.rc = MIB_E_OUT_OF_MEMORY;
  if (hipMemcpyAsync(d, stage.data(), (size_t)up, hipMemcpyHostToDevice, use.st) != hipSuccess) return use.rc = MIB_E_NO_DEVICE;
  std::vector<SameDesc> descs(k);
  for (size_t i = 0; i < k; i++) descs[i] = SameDesc{d + at_a[i], d + at_b[i], (uint32_t)a[i].size};
  if ((use.rc = same_device(use.st, use.tm, use.m, descs, differ))) return use.rc;
  use.timed = true;
  return 0;
}

extern "C" int mib_woff2_encode_batch(const mib_span *sfnts, size_t k, const mib_woff2_enc_opts *o, mib_buf *woff2,
                                      int *status) {
  if (k == 0) return 0;
  if (woff2)
    for (size_t i = 0; i < k; i++) woff2[i].data = nullptr, woff2[i].size = 0;
  if (!sfnts || !woff2 || !status) return MIB_E_INVALID_ARG;
  for (size_t i = 0; i < k; i++)
    if (!sfnts[i].data && sfnts[i].size) return MIB_E_INVALID_ARG;
  const int rc = encode_batch(sfnts, k, o, woff2, status);
  for (size_t i = 0; i < k; i++)
    if (rc || status[i]) drop(&woff2[i]);
  return rc;
}

extern "C" int mib_woff2_encode(const uint8_t *sfnt, size_t n, const mib_woff2_enc_opts *o, mib_buf *woff2) {
  if (!woff2) return MIB_E_INVALID_ARG;
  woff2->data = nullptr;
  woff2->size = 0;
  if (!sfnt && n) return MIB_E_INVALID_ARG;
  const mib_span one{sfnt, n};
  int status = 0;
  const int rc = mib_woff2_encode_batch(&one, 1, o, woff2, &status);
  return rc ? rc : status;
}
