// A .woff2 file -> the sfnt it stands for, assembled on the GPU (DESIGN.md 4c "A whole file").
// The container is parsed on the host (woff2_file.h: the plan); the Brotli stream is decoded on
// the device into one buffer; glyf, loca and hmtx are reconstructed from it in device memory
// (woff2_inv.hip's cores); then two kernels lay the sfnt out:
//   sfnt_assemble_kernel   every table in one launch (blockIdx.y: the table, its tiles over
//                          blockIdx.x): copied to its place over the output's 16-byte granules,
//                          zero-padded to 4 bytes, head's checkSumAdjustment cleared, and summed
//                          as big-endian words while the bytes are in registers
//   sfnt_directory_kernel  one wave: offset table, the records in tag order with the sums as
//                          their checksums, the file's sum, head's checkSumAdjustment
// Between the upload of the file's compressed bytes and the download of the sfnt only the
// 36-byte transformed-glyf header, hhea's numberOfHMetrics and the reconstruct cores' totals and
// flags visit the host.  woff2_file.h's host_assemble states the same result serially.
#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "common.h"
#include "load16.h"
#include "woff2_dev.h"
#include "woff2_file.h"

namespace mib {
namespace woff2file {

constexpr int kWave = 64;
constexpr int kAsmThreads = 256;
constexpr uint64_t kAsmTile = (uint64_t)kAsmThreads * 16;
constexpr uint32_t kAsmSpread = 256;   // blocks per table at most (each walks its tiles)
constexpr uint32_t kNoZero = 0xFFFFFFFFu;

// One table of the launch.  dst_off is a multiple of 4; src has any alignment and 16 readable
// bytes of slack behind its allocation's last byte (load16.h).
struct AsmDesc {
  const uint8_t *src;
  uint32_t dst_off, len;
  uint32_t zero_at;   // head with its checkSumAdjustment: 8 (bytes 8..11 are stored as zero); else kNoZero
  uint32_t pad;
};
// One record of the directory, in tag order.
struct DirRec {
  uint32_t tag, table, dst_off, len;
};

__device__ __forceinline__ uint32_t be_word(uint32_t w) { return __builtin_bswap32(w); }

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
  for (int d = kWave / 2; d > 0; d >>= 1) x += __shfl_xor(x, d, kWave);
  return x;
}

// Tiles are laid over the OUTPUT's 16-byte granules (out is 16-byte aligned), from the
// table's place in it: a granule whose 16 bytes are all the table's moves as one vector, its
// unaligned source read through load16_any; the head and tail granules, and the zero padding
// up to the 4-byte boundary, move byte by byte, so two tables that share a granule never touch
// each other's bytes.  The table's offset is a multiple of 4, so a granule's words are the
// table's words: each thread sums its granule's, a wave adds its lanes' sums with cross-lane
// adds and one lane adds the wave's into the table's sum.  The sum wraps, so the order of the
// adds does not matter.
__global__ __launch_bounds__(kAsmThreads) void sfnt_assemble_kernel(const AsmDesc *descs, uint8_t *out, uint32_t *sums) {
  const AsmDesc d = descs[blockIdx.y];
  const uint32_t padded = (d.len + 3) & ~3u;   // (len <= 2^32 - 4: woff2_file.h layout)
  const uint32_t mis = d.dst_off & 15;
  const uint64_t tiles = padded ? ((uint64_t)padded + mis + kAsmTile - 1) / kAsmTile : 0;
  uint8_t *dst = out + d.dst_off;
  uint32_t acc = 0;
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t lo = (int64_t)(16 * (t * kAsmThreads + threadIdx.x)) - (int64_t)mis;   // the granule's first byte in the table
    if (lo >= (int64_t)padded) continue;
    if (lo >= 0 && (uint64_t)lo + 16 <= d.len) {
      uint4 v = load16_any(d.src + lo);
      if (d.zero_at != kNoZero && lo <= (int64_t)d.zero_at && (int64_t)d.zero_at < lo + 16) {
        const int w = (int)(d.zero_at - (uint32_t)lo) >> 2;   // (both multiples of 4 apart)
        if (w == 0) v.x = 0;
        else if (w == 1) v.y = 0;
        else if (w == 2) v.z = 0;
        else v.w = 0;
      }
      *reinterpret_cast<uint4 *>(dst + lo) = v;
      acc += be_word(v.x) + be_word(v.y) + be_word(v.z) + be_word(v.w);
    } else {
#pragma unroll
      for (int w = 0; w < 4; w++) {
        uint32_t word = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int64_t at = lo + 4 * w + q;
          if (at < 0 || at >= (int64_t)padded) continue;   // another table's byte, or past the padding
          uint32_t b = at < (int64_t)d.len ? d.src[at] : 0;
          if (d.zero_at != kNoZero && (uint64_t)at - d.zero_at < 4) b = 0;
          dst[at] = (uint8_t)b;
          word |= b << (24 - 8 * q);
        }
        acc += word;
      }
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & (kWave - 1)) == 0 && acc) atomicAdd(&sums[blockIdx.y], acc);
}

// One wave.  The offset table and the records (their place, 12 + 16 r, is a multiple of 4: four
// word stores each); every lane sums the words it writes and its records' table sums, the
// wave's total is the file's sum, and head's checkSumAdjustment follows from it.
__global__ __launch_bounds__(kWave) void sfnt_directory_kernel(uint32_t flavor, uint32_t num, uint32_t range, uint32_t selector,
                                                              uint32_t shift, const DirRec *recs, const uint32_t *sums,
                                                              uint32_t adjust_at, uint8_t *out) {
  const int lane = threadIdx.x;
  uint32_t *o = reinterpret_cast<uint32_t *>(out);
  uint32_t acc = 0;
  if (lane == 0) {
    const uint32_t w0 = flavor, w1 = (num << 16) | range, w2 = (selector << 16) | shift;
    o[0] = be_word(w0);
    o[1] = be_word(w1);
    o[2] = be_word(w2);
    acc = w0 + w1 + w2;
  }
  for (uint32_t r = lane; r < num; r += kWave) {
    const DirRec rec = recs[r];
    const uint32_t cs = sums[rec.table];
    uint32_t *p = o + 3 + 4 * (size_t)r;
    p[0] = be_word(rec.tag);
    p[1] = be_word(cs);
    p[2] = be_word(rec.dst_off);
    p[3] = be_word(rec.len);
    acc += rec.tag + cs + rec.dst_off + rec.len + cs;   // the record's words, and the table's own
  }
  acc = wave_sum(acc);
  if (lane == 0 && adjust_at != kNoZero) *reinterpret_cast<uint32_t *>(out + adjust_at) = be_word(kHeadMagic - acc);
}

}  // namespace woff2file
}  // namespace mib

using namespace mib::woff2file;
using mib::woff2dev::DevMem;
using mib::woff2dev::Timer;

namespace {

struct AsmHost {   // what the launch uploads: the caller keeps it until the stream is synchronised
  std::vector<AsmDesc> descs;
  std::vector<DirRec> recs;
};

// The two kernels over a plan that has been laid out.  src[i]: table i's bytes on the device.
// The sfnt is left at *d_sfnt (in m); nothing is synchronised.
int assemble_device(hipStream_t st, Timer &tm, DevMem &m, const Plan &pl, const std::vector<const uint8_t *> &src,
                    AsmHost &host, uint8_t **d_sfnt) {
  const uint32_t num = (uint32_t)pl.t.size();
  std::vector<AsmDesc> &descs = host.descs;
  std::vector<DirRec> &recs = host.recs;
  descs.resize(num);
  recs.resize(num);
  uint64_t most = 1;
  for (uint32_t i = 0; i < num; i++) {
    const Table &t = pl.t[i];
    descs[i] = AsmDesc{src[i], t.dst_off, t.dst_len, i == pl.head && head_adjusted(pl) ? 8u : kNoZero, 0};
    const uint64_t tiles = ((uint64_t)t.dst_len + 3 + (t.dst_off & 15) + kAsmTile - 1) / kAsmTile;
    most = tiles > most ? tiles : most;
  }
  for (uint32_t r = 0; r < num; r++) {
    const Table &t = pl.t[pl.order[r]];
    recs[r] = DirRec{t.tag, pl.order[r], t.dst_off, t.dst_len};
  }
  AsmDesc *d_descs = m.take<AsmDesc>(num);
  DirRec *d_recs = m.take<DirRec>(num);
  uint32_t *d_sums = m.take<uint32_t>(num);
  uint8_t *d_out = m.take<uint8_t>((size_t)pl.sfnt_len);
  if (!d_descs || !d_recs || !d_sums || !d_out) return MIB_E_OUT_OF_MEMORY;
  if (hipMemcpyAsync(d_descs, descs.data(), sizeof(AsmDesc) * num, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(d_recs, recs.data(), sizeof(DirRec) * num, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemsetAsync(d_sums, 0, sizeof(uint32_t) * num, st) != hipSuccess)
    return MIB_E_NO_DEVICE;
  const uint32_t blocks = (uint32_t)(most < kAsmSpread ? most : kAsmSpread);
  tm.start("w2file_assemble");
  hipLaunchKernelGGL(sfnt_assemble_kernel, dim3(blocks, num), dim3(kAsmThreads), 0, st, d_descs, d_out, d_sums);
  tm.stop();
  uint32_t range, selector, shift;
  search_fields(num, &range, &selector, &shift);
  tm.start("w2file_directory");
  hipLaunchKernelGGL(sfnt_directory_kernel, dim3(1), dim3(kWave), 0, st, pl.flavor, num, range, selector & 0xFFFF, shift,
                     d_recs, d_sums, head_adjusted(pl) ? pl.t[pl.head].dst_off + 8 : kNoZero, d_out);
  tm.stop();
  if (hipGetLastError() != hipSuccess) return MIB_E_NO_DEVICE;
  *d_sfnt = d_out;
  return 0;
}

int download(hipStream_t st, const uint8_t *d_sfnt, size_t n, mib_buf *sfnt) {
  sfnt->data = mib_buf_alloc(n);
  if (!sfnt->data) {
    hipStreamSynchronize(st);
    return MIB_E_OUT_OF_MEMORY;
  }
  sfnt->size = n;
  hipMemcpyAsync(sfnt->data, d_sfnt, n, hipMemcpyDeviceToHost, st);
  return hipStreamSynchronize(st) == hipSuccess ? 0 : MIB_E_NO_DEVICE;
}

struct DefaultCall {   // the default context for one call: lock, device, stream, timer
  mib_ctx *c;
  hipStream_t st;
  DefaultCall() {
    mib_default_lock(1);
    c = mib_default_ctx();
    st = nullptr;
    if (c) {
      hipSetDevice(mib_ctx_device_of(c));
      st = (hipStream_t)mib_ctx_stream_of(c);
    }
  }
  ~DefaultCall() { mib_default_lock(0); }
};

void drop(mib_buf *b) {
  if (b->data) mib_buf_free(b);
  b->data = nullptr;
  b->size = 0;
}

}  // namespace

extern "C" int mib_woff2_decode(const uint8_t *woff2, size_t n, mib_buf *sfnt) {
  if (!sfnt) return MIB_E_INVALID_ARG;
  sfnt->data = nullptr;
  sfnt->size = 0;
  Plan pl;
  if (!parse(woff2, n, &pl)) return MIB_E_INVALID_ARG;   // (before anything is allocated on the device)
  DefaultCall use;   // (the lock is recursive: mib_ctx_decode below runs on this context inside it)
  if (!use.c) return MIB_E_NO_DEVICE;
  hipStream_t st = use.st;
  int rc = 0;
  bool timed = false;
  DevMem m;
  AsmHost host;
  Timer tm{use.c, st, false, {}};
  do {
    uint8_t *d_comp = m.take<uint8_t>(pl.comp_len), *d_stream = m.take<uint8_t>((size_t)pl.stream_len);
    if (!d_comp || !d_stream) {
      rc = MIB_E_OUT_OF_MEMORY;
      break;
    }
    if (pl.comp_len && hipMemcpyAsync(d_comp, woff2 + pl.comp_off, pl.comp_len, hipMemcpyHostToDevice, st) != hipSuccess) {
      rc = MIB_E_NO_DEVICE;
      break;
    }
    // the stream has to decode to exactly the directory's total: that is its capacity
    const uint64_t in_off[2] = {0, pl.comp_len}, out_off[2] = {0, pl.stream_len};
    int64_t size = 0;
    int status = 0;
    rc = mib_ctx_decode(use.c, d_comp, in_off, 1, d_stream, out_off, &size, &status, st);
    if (rc == 0 || rc == MIB_E_NEED_SPACE) rc = status;
    if (rc == MIB_E_NEED_SPACE || (rc == 0 && (uint64_t)size != pl.stream_len)) rc = MIB_E_INVALID_ARG;
    if (rc) break;
    // (mib_ctx_decode starts the context's kernel times afresh; this call's own follow it)
    tm.on = mib_ctx_profiling(use.c) == 1;
    uint8_t *d_glyf = nullptr, *d_loca = nullptr, *d_hmtx = nullptr;
    size_t glyf_b = 0, loca_b = 0, hmtx_b = 0;
    if (glyf_transformed(pl)) {
      const Table &g = pl.t[pl.glyf];
      uint8_t hdr[mib::woff2inv::kHeaderBytes];
      if (g.src_len < sizeof(hdr)) {
        rc = MIB_E_INVALID_ARG;
        break;
      }
      if (hipMemcpyAsync(hdr, d_stream + g.src_off, sizeof(hdr), hipMemcpyDeviceToHost, st) != hipSuccess ||
          hipStreamSynchronize(st) != hipSuccess) {
        rc = MIB_E_NO_DEVICE;
        break;
      }
      if ((rc = mib::woff2dev::reconstruct_glyf_device(st, tm, m, hdr, d_stream + g.src_off, g.src_len, &d_glyf, &glyf_b,
                                                       &d_loca, &loca_b)))
        break;
      if (hmtx_transformed(pl)) {
        const Table &h = pl.t[pl.hmtx];
        uint8_t nhm_be[2];
        if (hipMemcpyAsync(nhm_be, d_stream + pl.t[pl.hhea].src_off + 34, 2, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) {
          rc = MIB_E_NO_DEVICE;
          break;
        }
        const uint32_t ng = ((uint32_t)hdr[4] << 8) | hdr[5], nhm = ((uint32_t)nhm_be[0] << 8) | nhm_be[1];
        uint32_t long_loca = 0;
        if (!mib::woff2inv::hmtx_shape_ok(h.src_len, glyf_b, loca_b, ng, nhm, &long_loca)) {
          rc = MIB_E_INVALID_ARG;
          break;
        }
        if ((rc = mib::woff2dev::reconstruct_hmtx_device(st, tm, m, d_stream + h.src_off, h.src_len, d_glyf, glyf_b, d_loca,
                                                         long_loca, ng, nhm, &d_hmtx, &hmtx_b)))
          break;
      }
    }
    if (!layout(&pl, glyf_b, loca_b, hmtx_b)) {
      rc = MIB_E_INVALID_ARG;
      break;
    }
    std::vector<const uint8_t *> src(pl.t.size());
    for (size_t i = 0; i < pl.t.size(); i++) {
      const Table &t = pl.t[i];
      src[i] = t.kind == kGlyf ? d_glyf : t.kind == kLoca ? d_loca : t.kind == kHmtx ? d_hmtx : d_stream + t.src_off;
    }
    uint8_t *d_sfnt = nullptr;
    if ((rc = assemble_device(st, tm, m, pl, src, host, &d_sfnt))) break;
    if ((rc = download(st, d_sfnt, (size_t)pl.sfnt_len, sfnt))) break;
    timed = true;
  } while (0);
  if (rc) hipStreamSynchronize(st);   // nothing of this call is in flight when its buffers go
  tm.collect(timed);
  if (rc) drop(sfnt);
  return rc;
}

extern "C" int mib_debug_sfnt_assemble(uint32_t flavor, const uint32_t *tags, const mib_span *tables,
                                       const uint8_t *d_src_misalign, size_t k, mib_buf *sfnt) {
  if (!sfnt) return MIB_E_INVALID_ARG;
  sfnt->data = nullptr;
  sfnt->size = 0;
  if (k == 0 || k > 65535 || !tags || !tables) return MIB_E_INVALID_ARG;
  // the plan a file of these tables, all with the null transform, would give
  Plan pl;
  pl.flavor = flavor;
  pl.glyf = pl.loca = pl.hmtx = pl.hhea = pl.head = kNoTable;
  std::vector<size_t> at(k);   // each table's place in the source buffer
  size_t total = 0;
  for (size_t i = 0; i < k; i++) {
    if ((!tables[i].data && tables[i].size) || tables[i].size > mib::woff2inv::kMaxInput ||
        (d_src_misalign && d_src_misalign[i] > 15))
      return MIB_E_INVALID_ARG;
    if (d_src_misalign) total = ((total + 15) & ~(size_t)15) + d_src_misalign[i];
    at[i] = total;
    total += tables[i].size;
    if (total > mib::woff2inv::kMaxInput) return MIB_E_INVALID_ARG;
    pl.t.push_back(Table{tags[i], kCopy, (uint32_t)at[i], (uint32_t)tables[i].size, 0, 0});
    if (tags[i] == kHeadTag) pl.head = (uint32_t)i;
  }
  pl.stream_len = total;
  pl.order.resize(k);
  for (size_t i = 0; i < k; i++) pl.order[i] = (uint32_t)i;
  std::sort(pl.order.begin(), pl.order.end(), [&](uint32_t a, uint32_t b) { return pl.t[a].tag < pl.t[b].tag; });
  for (size_t i = 1; i < k; i++)
    if (pl.t[pl.order[i]].tag == pl.t[pl.order[i - 1]].tag) return MIB_E_INVALID_ARG;
  if (!layout(&pl, 0, 0, 0)) return MIB_E_INVALID_ARG;
  DefaultCall use;
  if (!use.c) return MIB_E_NO_DEVICE;
  hipStream_t st = use.st;
  int rc = 0;
  bool timed = false;
  DevMem m;
  AsmHost host;
  Timer tm{use.c, st, mib_ctx_profiling(use.c) == 1, {}};
  do {
    uint8_t *d_src = m.take<uint8_t>(total);
    if (!d_src) {
      rc = MIB_E_OUT_OF_MEMORY;
      break;
    }
    std::vector<const uint8_t *> src(k);
    bool ok = true;
    for (size_t i = 0; i < k; i++) {
      src[i] = d_src + at[i];
      if (tables[i].size)
        ok = ok && hipMemcpyAsync(d_src + at[i], tables[i].data, tables[i].size, hipMemcpyHostToDevice, st) == hipSuccess;
    }
    if (!ok) {
      rc = MIB_E_NO_DEVICE;
      break;
    }
    uint8_t *d_sfnt = nullptr;
    if ((rc = assemble_device(st, tm, m, pl, src, host, &d_sfnt))) break;
    if ((rc = download(st, d_sfnt, (size_t)pl.sfnt_len, sfnt))) break;
    timed = true;
  } while (0);
  if (rc) hipStreamSynchronize(st);
  tm.collect(timed);
  if (rc) drop(sfnt);
  return rc;
}
