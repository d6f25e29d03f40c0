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
#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "common.h"
#include "load16.h"
#include "woff2_batch.h"
#include "woff2_dev.h"
#include "woff2_write.h"

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

struct GroupFont {   // a font of the group whose plan parsed
  size_t slot;       // in the call's arrays
  Plan *pl;
  const uint8_t *d_font;
  GlyfSized gz;
  HmtxSized hz;
  bool alive;
  uint64_t stream_at;   // its stream in the group's stream buffer
};

// One group: fonts idx[0..n) of the call, all parsed.  Non-zero: the call fails.
int encode_group(mib_ctx *c, hipStream_t st, const mib_span *sfnts, std::vector<Plan> &plans, const size_t *idx, size_t n,
                 const mib_enc_opts &eo, mib_buf *woff2, int *status) {
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
    // the transforms' sizes, font after font, then each font's layout
    uint64_t stream_bytes = 0, bound = 0;
    for (size_t i = 0; i < n && !rc; i++) {
      GroupFont &f = fonts[i];
      f.slot = idx[i];
      f.pl = &plans[idx[i]];
      f.d_font = d_fonts + base[i];
      f.alive = true;
      f.gz.total = f.hz.total = 0;
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
      const uint32_t fix = head_fix(*f.pl);
      for (uint32_t i = 0; i < f.pl->t.size(); i++) {
        const Table &t = f.pl->t[i];
        if (t.state != kPlain || !t.len) continue;
        descs.push_back(PackDesc{f.d_font + t.src_off, f.stream_at + t.at, t.len, i == f.pl->head ? fix : (uint32_t)kHeadNone});
        const uint64_t tiles = ((uint64_t)t.len + 15 + kPackTile - 1) / kPackTile;
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
      if (!finish(*f.pl, sfnts[f.slot].data, comp, hdr)) {
        status[f.slot] = MIB_E_INVALID_ARG;
        continue;
      }
      mib_buf *b = &woff2[f.slot];
      const size_t total = (size_t)file_bytes(*f.pl, comp), dir_b = f.pl->dir.size();
      b->data = mib_buf_alloc(total);
      if (!b->data) {
        status[f.slot] = MIB_E_OUT_OF_MEMORY;
        continue;
      }
      b->size = total;
      memcpy(b->data, hdr, sizeof(hdr));
      memcpy(b->data + sizeof(hdr), f.pl->dir.data(), dir_b);
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
  std::vector<size_t> parsed;   // (before anything is allocated on the device)
  std::vector<uint64_t> lens;
  for (size_t i = 0; i < k; i++) {
    status[i] = parse(sfnts[i].data, sfnts[i].size, transforms, &plans[i]) == kOk ? 0 : MIB_E_INVALID_ARG;
    if (status[i]) continue;
    parsed.push_back(i);
    lens.push_back(sfnts[i].size);
  }
  if (parsed.empty()) return 0;
  Call use(false);   // (every group has its own timer and buffers)
  if (!use.c) return MIB_E_NO_DEVICE;
  for (const mib::woff2file::Group &g : mib::woff2file::make_groups(lens, mib::woff2file::forced_group_bytes()))
    if ((use.rc = encode_group(use.c, use.st, sfnts, plans, &parsed[g.first], g.count, eo, woff2, status))) break;
  return use.rc;
}

}  // namespace

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
