// A .woff2 file -> the sfnt it stands for, assembled on the GPU (DESIGN.md 4c "A whole file").
// The container is parsed on the host (woff2_file.h: the plan); the Brotli stream is decoded on
// the device into one buffer; glyf, loca and hmtx are reconstructed from it in device memory
// (woff2_inv.hip's cores); then two kernels lay the sfnt out:
//   sfnt_assemble_kernel   every table in one launch (blockIdx.x: the table, its tiles over
//                          blockIdx.y): copied to its place over the output's 16-byte granules,
//                          zero-padded to 4 bytes, head's checkSumAdjustment cleared, and summed
//                          as big-endian words while the bytes are in registers
//   sfnt_directory_kernel  one wave a font: offset table, the records in tag order with the sums
//                          as their checksums, the file's sum, head's checkSumAdjustment
// Between the upload of the file's compressed bytes and the download of the sfnt only the
// 36-byte transformed-glyf header, hhea's numberOfHMetrics and the reconstruct cores' totals and
// flags visit the host.  woff2_file.h's host_assemble states the same result serially.
//
// mib_woff2_decode_batch works k files in shared launches (DESIGN.md 4c "A batch of files";
// woff2_batch.h decides where the bytes go): per group of files one upload, one decode call over
// every stream, one w2file_peek launch and read-back for the headers, the glyf reconstruct per
// font, one hmtx launch, one launch of each assembly kernel over every font, and one
// synchronisation for the downloads.  Each decode call starts the context's kernel times afresh:
// after a call of more than one group the times reported are the last group's.
// mib_woff2_decode is the batch with k = 1, and mib_debug_sfnt_assemble is
// mib_debug_sfnt_assemble_batch with one font: one code path each.
//
// A font collection (flavor ttcf; DESIGN.md 4c "A font collection") is one file of a group like
// any other and comes out as its TTC: a peek row and a reconstruct per transformed glyf / loca
// pair, an hmtx unit of the group's one hmtx launch per transformed hmtx, a descriptor of the
// assembly launch per table that a member lists, and a wave of the directory launch per member,
// which writes its directory behind the TTC header and its own word of that header.
// mib_debug_ttc_assemble runs the two assembly kernels alone over one collection.
#include <hip/hip_runtime.h>
#include <string.h>

#include <chrono>
#include <vector>

#include "common.h"
#include "load16.h"
#include "woff2_batch.h"
#include "woff2_dev.h"
#include "woff2_file.h"

namespace mib {
namespace woff2file {

constexpr int kWave = 64;
constexpr uint32_t kAsmSpread = 256;   // blocks per table at most (each walks its tiles)
constexpr uint32_t kPeekBytes = 40;    // a row of the peek: 36 + 2, padded

// One row of the peek: a transformed glyf table's first 36 bytes (a row per glyf / loca pair) or
// an hhea's bytes 34..35 (a row per hmtx unit); null: not wanted, the row's bytes are then zero.
struct PeekFont {
  const uint8_t *glyf, *hhea34;
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
// blockIdx.x: the table, of every font of the launch (a launch may hold more tables than the
// 65,535 of the other grid dimensions); blockIdx.y: its share of the table's tiles.
__global__ __launch_bounds__(kAsmThreads) void sfnt_assemble_kernel(const AsmDesc *descs, uint8_t *out, uint32_t *sums) {
  const AsmDesc d = descs[blockIdx.x];
  const uint32_t padded = (d.len + 3) & ~3u;   // (len <= 2^32 - 4: woff2_file.h layout)
  const uint32_t mis = d.dst_off & 15;         // (the font's base is a multiple of 16)
  const uint64_t tiles = padded ? ((uint64_t)padded + mis + kAsmTile - 1) / kAsmTile : 0;
  uint8_t *dst = out + d.out_base + d.dst_off;
  uint32_t acc = 0;
  for (uint64_t t = blockIdx.y; t < tiles; t += gridDim.y) {
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
  if ((threadIdx.x & (kWave - 1)) == 0 && acc) atomicAdd(&sums[d.sum], acc);
}

// One wave per font (blockIdx.x).  The offset table and the records (their place, 12 + 16 r, is a
// multiple of 4: four word stores each); every lane sums the words it writes and its records'
// table sums, the wave's total is the file's sum, and head's checkSumAdjustment follows from it.
// A member of a collection is a font here: its directory lies at dir_off in the TTC (a multiple
// of 4, not of 16: word stores throughout), its records reach the sums of tables that other
// members may list too, and it stores the shared head's checkSumAdjustment only where adjust_at
// says so (one wave per head: the same bytes on every run).  Each member stores its own word of
// the TTC header, member 0 the rest of it; the header takes part in no sum.
__global__ __launch_bounds__(kWave) void sfnt_directory_kernel(const DirFont *fonts, const DirRec *all_recs,
                                                              const uint32_t *all_sums, uint8_t *all_out) {
  const DirFont f = fonts[blockIdx.x];
  const DirRec *recs = all_recs + f.first_rec;
  const uint32_t *sums = all_sums + f.first_sum;
  uint8_t *file = all_out + f.out_base, *out = file + f.dir_off;
  const int lane = threadIdx.x;
  uint32_t *o = reinterpret_cast<uint32_t *>(out);
  if (f.ttc_index != kNoZero && lane == kWave - 1) {
    uint32_t *h = reinterpret_cast<uint32_t *>(file);
    h[3 + f.ttc_index] = be_word(f.dir_off);
    if (f.ttc_index == 0) {
      h[0] = be_word(kFlavorTtc);
      h[1] = be_word(f.ttc_version);
      h[2] = be_word(f.ttc_fonts);
      if (f.ttc_version == kTtcVersion2) h[3 + f.ttc_fonts] = h[4 + f.ttc_fonts] = h[5 + f.ttc_fonts] = 0;
    }
  }
  uint32_t acc = 0;
  if (lane == 0) {
    const uint32_t w0 = f.flavor, w1 = (f.num << 16) | f.range, w2 = (f.selector << 16) | f.shift;
    o[0] = be_word(w0);
    o[1] = be_word(w1);
    o[2] = be_word(w2);
    acc = w0 + w1 + w2;
  }
  for (uint32_t r = lane; r < f.num; r += kWave) {
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
  if (lane == 0 && f.adjust_at != kNoZero) *reinterpret_cast<uint32_t *>(file + f.adjust_at) = be_word(kHeadMagic - acc);
}

// A thread per font, in the shape of the decoder's peek_heads_kernel: what the host needs of every
// font's decoded stream before it can size the reconstructed tables, in one read-back.
__global__ void w2file_peek_kernel(const PeekFont *fonts, uint32_t k, uint8_t *rows) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < k; i += gridDim.x * blockDim.x) {
    const PeekFont f = fonts[i];
    uint8_t *row = rows + (size_t)kPeekBytes * i;
    for (int q = 0; q < 36; q++) row[q] = f.glyf ? f.glyf[q] : 0;
    for (int q = 0; q < 2; q++) row[36 + q] = f.hhea34 ? f.hhea34[q] : 0;
    row[38] = row[39] = 0;
  }
}

}  // namespace woff2file
}  // namespace mib

using namespace mib::woff2file;
using mib::woff2dev::Call;
using mib::woff2dev::DevMem;
using mib::woff2dev::drop;
using mib::woff2dev::HmtxFont;
using mib::woff2dev::Timer;

extern "C" int mib_ctx_decode_caps(mib_ctx *c, const uint8_t *d_in, const uint64_t *in_offsets, size_t k, uint8_t *d_out,
                                   const uint64_t *out_offsets, const uint64_t *out_caps, int64_t *out_sizes, int *status,
                                   void *stream);

namespace {

uint64_t g_group_bytes = 0;      // mib_force_woff2_group_bytes (0: woff2_batch.h's default)
double g_batch_ms[2] = {0, 0};   // the last batch call: the per-font glyf loop, the whole call (host wall time)

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// The two kernels over the fonts of a launch (at least one).  src of every descriptor: the
// table's bytes on the device.  The output buffer (l.out_bytes; font f at its out_base) is left
// at *d_out_p (in m); nothing is synchronised, and the caller keeps `l` until the stream is.
int assemble_device(hipStream_t st, Timer &tm, DevMem &m, const Launch &l, uint8_t **d_out_p) {
  const size_t nt = l.descs.size(), nr = l.recs.size(), nf = l.fonts.size();   // (nr != nt: a collection's shared tables)
  AsmDesc *d_descs = m.take<AsmDesc>(nt);
  DirRec *d_recs = m.take<DirRec>(nr);
  DirFont *d_fonts = m.take<DirFont>(nf);
  uint32_t *d_sums = m.take<uint32_t>(nt);
  uint8_t *d_out = m.take<uint8_t>((size_t)l.out_bytes);
  if (!d_descs || !d_recs || !d_fonts || !d_sums || !d_out) return MIB_E_OUT_OF_MEMORY;
  if (hipMemcpyAsync(d_descs, l.descs.data(), sizeof(AsmDesc) * nt, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(d_recs, l.recs.data(), sizeof(DirRec) * nr, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(d_fonts, l.fonts.data(), sizeof(DirFont) * nf, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemsetAsync(d_sums, 0, sizeof(uint32_t) * nt, st) != hipSuccess)
    return MIB_E_NO_DEVICE;
  const uint32_t spread = (uint32_t)(l.most_tiles < kAsmSpread ? l.most_tiles : kAsmSpread);
  tm.start("w2file_assemble");
  hipLaunchKernelGGL(sfnt_assemble_kernel, dim3((uint32_t)nt, spread), dim3(kAsmThreads), 0, st, d_descs, d_out, d_sums);
  tm.stop();
  tm.start("w2file_directory");
  hipLaunchKernelGGL(sfnt_directory_kernel, dim3((uint32_t)nf), dim3(kWave), 0, st, d_fonts, d_recs, d_sums, d_out);
  tm.stop();
  if (hipGetLastError() != hipSuccess) return MIB_E_NO_DEVICE;
  *d_out_p = d_out;
  return 0;
}

// The plan a file of these k tables, all with the null transform, would give, before layout().
// src_off: the table's place in the font's source bytes (misalign: from a 16-byte boundary on);
// stream_len: how many those are.
bool plan_sources(uint32_t flavor, const uint32_t *tags, const mib_span *tables, const uint8_t *misalign, size_t k, Plan *pl) {
  if (k == 0 || k > 65535) return false;
  pl->flavor = flavor;
  pl->t.clear();
  pl->glyf = pl->loca = pl->hmtx = pl->hhea = pl->head = kNoTable;
  size_t total = 0;
  for (size_t i = 0; i < k; i++) {
    if ((!tables[i].data && tables[i].size) || tables[i].size > mib::woff2inv::kMaxInput || (misalign && misalign[i] > 15))
      return false;
    if (misalign) total = ((total + 15) & ~(size_t)15) + misalign[i];
    const size_t at = total;
    total += tables[i].size;
    if (total > mib::woff2inv::kMaxInput) return false;
    pl->t.push_back(Table{tags[i], kCopy, (uint32_t)at, (uint32_t)tables[i].size, 0, 0});
    if (tags[i] == kHeadTag) pl->head = (uint32_t)i;
  }
  pl->stream_len = total;
  return true;
}

// The same tables as a collection's directory (repeated tags allowed), listed by n_fonts members:
// member f has counts[f] tables, its indices taken in order from `indices`.  Laid out.
bool plan_of_collection(uint32_t version, const uint32_t *tags, const mib_span *tables, const uint8_t *misalign, size_t k,
                        const uint32_t *flavors, const uint32_t *counts, const uint32_t *indices, size_t n_fonts, Plan *pl) {
  if ((version != kTtcVersion1 && version != kTtcVersion2) || n_fonts == 0 || n_fonts > 65535) return false;
  if (!plan_sources(kFlavorTtc, tags, tables, misalign, k, pl)) return false;
  pl->head = kNoTable;
  pl->ttc_version = version;
  pl->fonts.clear();
  uint64_t dirs = 0;
  size_t first = 0;
  for (size_t f = 0; f < n_fonts; f++) {
    dirs += 12 + 16 * (uint64_t)counts[f];
    if (counts[f] == 0 || dirs > kMaxDirectoryBytes) return false;
    pl->fonts.push_back(Member{flavors[f], {}, kNoTable, false, 0});
    for (uint32_t i = 0; i < counts[f]; i++) {
      if (indices[first + i] >= k) return false;
      pl->fonts.back().order.push_back(indices[first + i]);
    }
    first += counts[f];
  }
  pl->pairs.clear();
  pl->hunits.clear();
  pl->unit.assign(k, kNoTable);
  return collection_members(pl) && layout_units(pl, nullptr, nullptr, nullptr);
}

bool plan_of_tables(uint32_t flavor, const uint32_t *tags, const mib_span *tables, const uint8_t *misalign, size_t k,
                    Plan *pl) {
  if (!plan_sources(flavor, tags, tables, misalign, k, pl)) return false;
  pl->order.resize(k);
  for (size_t i = 0; i < k; i++) pl->order[i] = (uint32_t)i;
  std::sort(pl->order.begin(), pl->order.end(), [&](uint32_t a, uint32_t b) { return pl->t[a].tag < pl->t[b].tag; });
  for (size_t i = 1; i < k; i++)
    if (pl->t[pl->order[i]].tag == pl->t[pl->order[i - 1]].tag) return false;
  return layout(pl, 0, 0, 0);
}

struct BatchFont {   // a file of the group whose stream decoded: a single font or a collection
  size_t slot;       // in the call's arrays
  Plan *pl;
  const uint8_t *d_stream;
  size_t row0;       // its rows of the peek: one per pair, then one per hmtx unit
  std::vector<const uint8_t *> glyfs, locas, hmtxs;   // device: per pair, per pair, per hmtx unit
  std::vector<uint64_t> glyf_b, loca_b, hmtx_b;
  std::vector<long> hm;   // per hmtx unit: its place in the hmtx launch, or -1
  uint64_t out_base;
  bool alive;
};

// One group: files idx[0..n) of the call, all parsed.  Non-zero: the call fails.
int decode_group(mib_ctx *c, hipStream_t st, const mib_span *files, std::vector<Plan> &plans, const size_t *idx, size_t n,
                 mib_buf *sfnt, int *status) {
  std::vector<const Plan *> pp(n);
  for (size_t i = 0; i < n; i++) pp[i] = &plans[idx[i]];
  const StreamPack pack = pack_streams(pp.data(), n);
  std::vector<uint8_t> comp((size_t)pack.in_off[n]);
  for (size_t i = 0; i < n; i++)
    if (pp[i]->comp_len) memcpy(comp.data() + pack.in_off[i], files[idx[i]].data + pp[i]->comp_off, pp[i]->comp_len);
  // what the launches read from the host until the stream is synchronised
  std::vector<int64_t> sizes(n);
  std::vector<int> dec(n);
  std::vector<BatchFont> fonts;
  std::vector<PeekFont> peek;
  std::vector<uint8_t> rows;
  std::vector<HmtxFont> hm;
  std::vector<int> hm_bad;
  Launch launch;
  int rc = 0;
  bool timed = false;
  DevMem gm;   // the group's buffers: streams, reconstructed tables, outputs
  Timer tm{c, st, false, {}};
  do {
    uint8_t *d_comp = gm.take<uint8_t>(comp.size()), *d_streams = gm.take<uint8_t>((size_t)pack.stream_bytes);
    if (!d_comp || !d_streams) {
      rc = MIB_E_OUT_OF_MEMORY;
      break;
    }
    if (!comp.empty() && hipMemcpyAsync(d_comp, comp.data(), comp.size(), hipMemcpyHostToDevice, st) != hipSuccess) {
      rc = MIB_E_NO_DEVICE;
      break;
    }
    // every stream has to decode to exactly its directory's total: that is its capacity
    rc = mib_ctx_decode_caps(c, d_comp, pack.in_off.data(), n, d_streams, pack.slot_off.data(), pack.cap.data(),
                             sizes.data(), dec.data(), st);
    if (rc && rc != MIB_E_NEED_SPACE) break;
    rc = 0;
    tm.on = mib_ctx_profiling(c) == 1;   // (the decode started the context's kernel times afresh)
    for (size_t i = 0; i < n; i++) {
      int s = dec[i];
      if (s == MIB_E_NEED_SPACE || (s == 0 && (uint64_t)sizes[i] != pp[i]->stream_len)) s = MIB_E_INVALID_ARG;
      status[idx[i]] = s;
      if (s) continue;
      Plan *pl = &plans[idx[i]];
      bool short_glyf = false;
      for (const Pair &p : pl->pairs) short_glyf |= pl->t[p.glyf].src_len < (uint32_t)mib::woff2inv::kHeaderBytes;
      if (short_glyf) {
        status[idx[i]] = MIB_E_INVALID_ARG;
        continue;
      }
      BatchFont f;
      f.slot = idx[i];
      f.pl = pl;
      f.d_stream = d_streams + pack.slot_off[i];
      f.row0 = 0;
      f.glyfs.assign(pl->pairs.size(), nullptr);
      f.locas.assign(pl->pairs.size(), nullptr);
      f.hmtxs.assign(pl->hunits.size(), nullptr);
      f.glyf_b.assign(pl->pairs.size(), 0);
      f.loca_b.assign(pl->pairs.size(), 0);
      f.hmtx_b.assign(pl->hunits.size(), 0);
      f.hm.assign(pl->hunits.size(), -1);
      f.out_base = 0;
      f.alive = true;
      fonts.push_back(std::move(f));
    }
    // the headers the host sizes the reconstructed tables from: one launch, one read-back; a row
    // per transformed glyf pair (the table's header) and per hmtx unit (its hhea's numberOfHMetrics)
    for (BatchFont &f : fonts) {
      f.row0 = peek.size();
      for (const Pair &p : f.pl->pairs) peek.push_back(PeekFont{f.d_stream + f.pl->t[p.glyf].src_off, nullptr});
      for (const HmtxUnit &u : f.pl->hunits) peek.push_back(PeekFont{nullptr, f.d_stream + f.pl->t[u.hhea].src_off + 34});
    }
    if (!peek.empty()) {
      PeekFont *d_peek = gm.take<PeekFont>(peek.size());
      uint8_t *d_rows = gm.take<uint8_t>(kPeekBytes * peek.size());
      if (!d_peek || !d_rows) {
        rc = MIB_E_OUT_OF_MEMORY;
        break;
      }
      rows.resize(kPeekBytes * peek.size());
      hipMemcpyAsync(d_peek, peek.data(), sizeof(PeekFont) * peek.size(), hipMemcpyHostToDevice, st);
      tm.start("w2file_peek");
      hipLaunchKernelGGL(w2file_peek_kernel, dim3((uint32_t)((peek.size() + 255) / 256)), dim3(256), 0, st, d_peek,
                         (uint32_t)peek.size(), d_rows);
      tm.stop();
      hipMemcpyAsync(rows.data(), d_rows, rows.size(), hipMemcpyDeviceToHost, st);
      if (hipStreamSynchronize(st) != hipSuccess) {
        rc = MIB_E_NO_DEVICE;
        break;
      }
    }
    // glyf and loca, pair after pair: a pair's temporaries go before the next one's come
    const auto loop0 = std::chrono::steady_clock::now();
    for (BatchFont &f : fonts) {
      for (size_t p = 0; p < f.pl->pairs.size() && f.alive && !rc; p++) {
        const Table &g = f.pl->t[f.pl->pairs[p].glyf];
        DevMem tmp;
        uint8_t *d_glyf = nullptr, *d_loca = nullptr;
        size_t glyf_b = 0, loca_b = 0;
        const int r = mib::woff2dev::reconstruct_glyf_device(st, tm, tmp, gm, rows.data() + kPeekBytes * (f.row0 + p),
                                                             f.d_stream + g.src_off, g.src_len, &d_glyf, &glyf_b, &d_loca, &loca_b);
        hipStreamSynchronize(st);   // (its last kernels read the temporaries)
        f.glyfs[p] = d_glyf, f.locas[p] = d_loca, f.glyf_b[p] = glyf_b, f.loca_b[p] = loca_b;
        if (r == MIB_E_NO_DEVICE) {
          rc = r;
        } else if (r) {
          status[f.slot] = r;
          f.alive = false;
        }
      }
      if (rc) break;
    }
    g_batch_ms[0] += ms_since(loop0);
    if (rc) break;
    // hmtx: every unit of every file, in one launch
    size_t hm_bytes = 0;
    uint32_t most_ng = 0;
    std::vector<size_t> hm_at;
    for (BatchFont &f : fonts) {
      const size_t np = f.pl->pairs.size(), first = hm.size(), bytes0 = hm_bytes;
      for (size_t u = 0; u < f.pl->hunits.size() && f.alive; u++) {
        const HmtxUnit &hu = f.pl->hunits[u];
        const Table &h = f.pl->t[hu.hmtx];
        const uint8_t *hdr = rows.data() + kPeekBytes * (f.row0 + hu.pair), *hh = rows.data() + kPeekBytes * (f.row0 + np + u);
        const uint32_t ng = ((uint32_t)hdr[4] << 8) | hdr[5], nhm = ((uint32_t)hh[36] << 8) | hh[37];
        uint32_t long_loca = 0;
        if (!mib::woff2inv::hmtx_shape_ok(h.src_len, f.glyf_b[hu.pair], f.loca_b[hu.pair], ng, nhm, &long_loca)) {
          status[f.slot] = MIB_E_INVALID_ARG;
          f.alive = false;
          break;
        }
        f.hm[u] = (long)hm.size();
        f.hmtx_b[u] = 4 * (uint64_t)nhm + 2 * (uint64_t)(ng - nhm);
        hm.push_back(HmtxFont{f.d_stream + h.src_off, h.src_len, f.glyfs[hu.pair], f.locas[hu.pair], nullptr,
                              (uint32_t)f.glyf_b[hu.pair], long_loca, ng, nhm});
        hm_at.push_back(hm_bytes);
        hm_bytes = (hm_bytes + (size_t)f.hmtx_b[u] + 15) & ~(size_t)15;
        most_ng = ng > most_ng ? ng : most_ng;
      }
      if (!f.alive) {   // a rejected file's units leave the launch (most_ng may stay above what is left)
        hm.resize(first);
        hm_at.resize(first);
        hm_bytes = bytes0;
      }
    }
    int *d_hm_bad = nullptr;
    if (!hm.empty()) {
      uint8_t *d_hm_out = gm.take<uint8_t>(hm_bytes);
      HmtxFont *d_hm = gm.take<HmtxFont>(hm.size());
      d_hm_bad = gm.take<int>(hm.size());
      if (!d_hm_out || !d_hm || !d_hm_bad) {
        rc = MIB_E_OUT_OF_MEMORY;
        break;
      }
      for (size_t q = 0; q < hm.size(); q++) hm[q].out = d_hm_out + hm_at[q];
      for (BatchFont &f : fonts)
        for (size_t u = 0; u < f.hm.size() && f.alive; u++) f.hmtxs[u] = hm[(size_t)f.hm[u]].out;
      hm_bad.assign(hm.size(), 0);
      hipMemsetAsync(d_hm_bad, 0, sizeof(int) * hm.size(), st);
      hipMemcpyAsync(d_hm, hm.data(), sizeof(HmtxFont) * hm.size(), hipMemcpyHostToDevice, st);
      mib::woff2dev::launch_hmtx(st, tm, d_hm, hm.size(), most_ng, d_hm_bad);
    }
    // layout per file, then the two assembly kernels once over every font of every file
    for (BatchFont &f : fonts) {
      if (!f.alive) continue;
      const FontSrc src{f.d_stream, f.glyfs.empty() ? nullptr : f.glyfs[0], f.locas.empty() ? nullptr : f.locas[0],
                        f.hmtxs.empty() ? nullptr : f.hmtxs[0], f.glyfs.data(), f.locas.data(), f.hmtxs.data()};
      if (!layout_units(f.pl, f.glyf_b.data(), f.loca_b.data(), f.hmtx_b.data()) || !add_font(&launch, *f.pl, src)) {
        status[f.slot] = MIB_E_INVALID_ARG;
        f.alive = false;
        continue;
      }
      f.out_base = launch.fonts.back().out_base;
    }
    if (!launch.fonts.empty()) {
      uint8_t *d_out = nullptr;
      if ((rc = assemble_device(st, tm, gm, launch, &d_out))) break;
      for (BatchFont &f : fonts) {
        if (!f.alive) continue;
        mib_buf *b = &sfnt[f.slot];
        b->data = mib_buf_alloc((size_t)f.pl->sfnt_len);
        if (!b->data) {
          status[f.slot] = MIB_E_OUT_OF_MEMORY;
          f.alive = false;
          continue;
        }
        b->size = (size_t)f.pl->sfnt_len;
        hipMemcpyAsync(b->data, d_out + f.out_base, b->size, hipMemcpyDeviceToHost, st);
      }
    }
    if (d_hm_bad) hipMemcpyAsync(hm_bad.data(), d_hm_bad, sizeof(int) * hm.size(), hipMemcpyDeviceToHost, st);
    if (hipStreamSynchronize(st) != hipSuccess) {
      rc = MIB_E_NO_DEVICE;
      break;
    }
    // flags that do not fit the size; a loca entry that does not fit the glyf table
    for (BatchFont &f : fonts)
      for (size_t u = 0; u < f.hm.size() && f.alive; u++)
        if (hm_bad[(size_t)f.hm[u]]) {
          drop(&sfnt[f.slot]);
          status[f.slot] = MIB_E_INVALID_ARG;
          f.alive = false;
        }
    timed = true;
  } while (0);
  if (rc) hipStreamSynchronize(st);   // nothing of this group is in flight when its buffers go
  tm.collect(timed);
  return rc;
}

}  // namespace

extern "C" int mib_woff2_decode_batch(const mib_span *files, size_t k, mib_buf *sfnt, int *status) {
  if (k == 0) return 0;
  if (sfnt)
    for (size_t i = 0; i < k; i++) sfnt[i].data = nullptr, sfnt[i].size = 0;
  if (!files || !sfnt || !status) return MIB_E_INVALID_ARG;
  for (size_t i = 0; i < k; i++)
    if (!files[i].data && files[i].size) return MIB_E_INVALID_ARG;
  const auto call0 = std::chrono::steady_clock::now();
  std::vector<Plan> plans(k);
  std::vector<size_t> parsed;   // (before anything is allocated on the device)
  std::vector<uint64_t> lens;
  for (size_t i = 0; i < k; i++) {
    status[i] = parse(files[i].data, files[i].size, &plans[i]) ? 0 : MIB_E_INVALID_ARG;
    if (status[i]) continue;
    parsed.push_back(i);
    lens.push_back(plans[i].stream_len);
  }
  if (parsed.empty()) return 0;
  Call use(false);   // (every group has its own timer and buffers)
  if (!use.c) return MIB_E_NO_DEVICE;
  g_batch_ms[0] = 0;
  for (const Group &g : make_groups(lens, g_group_bytes))
    if ((use.rc = decode_group(use.c, use.st, files, plans, &parsed[g.first], g.count, sfnt, status))) break;
  if (use.rc)
    for (size_t i = 0; i < k; i++) drop(&sfnt[i]);
  g_batch_ms[1] = ms_since(call0);
  return use.rc;
}

extern "C" int mib_woff2_decode(const uint8_t *woff2, size_t n, mib_buf *sfnt) {
  if (!sfnt) return MIB_E_INVALID_ARG;
  sfnt->data = nullptr;
  sfnt->size = 0;
  if (!woff2 && n) return MIB_E_INVALID_ARG;
  const mib_span one{woff2, n};
  int status = 0;
  const int rc = mib_woff2_decode_batch(&one, 1, sfnt, &status);
  return rc ? rc : status;
}

extern "C" void mib_force_woff2_group_bytes(uint64_t bytes) { g_group_bytes = bytes; }
uint64_t mib::woff2file::forced_group_bytes() { return g_group_bytes; }   // (the writer's groups: woff2_write.hip)

// diagnostic (DESIGN.md's measurements): host wall time of the last mib_woff2_decode_batch or
// mib_woff2_decode (the batch with k = 1) that reached the device -- its per-font glyf
// reconstruct loops, and the whole call
extern "C" void mib_woff2_batch_last_ms(double out[2]) {
  out[0] = g_batch_ms[0];
  out[1] = g_batch_ms[1];
}

extern "C" int mib_debug_sfnt_assemble_batch(const uint32_t *flavors, const uint32_t *counts, const uint32_t *tags,
                                             const mib_span *tables, const uint8_t *d_src_misalign, size_t k, mib_buf *sfnt) {
  if (k == 0) return 0;
  if (sfnt)
    for (size_t f = 0; f < k; f++) sfnt[f].data = nullptr, sfnt[f].size = 0;
  if (!flavors || !counts || !tags || !tables || !sfnt) return MIB_E_INVALID_ARG;
  // every font's source bytes from a 16-byte boundary of one buffer on, staged on the host
  std::vector<Plan> plans(k);
  std::vector<size_t> base(k);
  size_t first = 0, total = 0;
  for (size_t f = 0; f < k; f++) {
    if (!plan_of_tables(flavors[f], tags + first, tables + first, d_src_misalign ? d_src_misalign + first : nullptr, counts[f],
                        &plans[f]))
      return MIB_E_INVALID_ARG;
    base[f] = total = (total + 15) & ~(size_t)15;
    total += (size_t)plans[f].stream_len;
    first += counts[f];
  }
  std::vector<uint8_t> stage(total);
  first = 0;
  for (size_t f = 0; f < k; f++) {
    for (size_t i = 0; i < counts[f]; i++)
      if (tables[first + i].size) memcpy(stage.data() + base[f] + plans[f].t[i].src_off, tables[first + i].data, tables[first + i].size);
    first += counts[f];
  }
  Launch host;   // (declared before the scope: the launches read it until the stream is synchronised)
  Call use(true);
  if (!use.c) return MIB_E_NO_DEVICE;
  uint8_t *d_src = use.m.take<uint8_t>(total), *d_out = nullptr;
  if (!d_src) return use.rc = MIB_E_OUT_OF_MEMORY;
  if (total && hipMemcpyAsync(d_src, stage.data(), total, hipMemcpyHostToDevice, use.st) != hipSuccess)
    return use.rc = MIB_E_NO_DEVICE;
  for (size_t f = 0; f < k; f++)
    if (!add_font(&host, plans[f], FontSrc{d_src + base[f], nullptr, nullptr, nullptr})) return use.rc = MIB_E_INVALID_ARG;
  if ((use.rc = assemble_device(use.st, use.tm, use.m, host, &d_out))) return use.rc;
  for (size_t f = 0; f < k; f++) {   // every font's download, then one synchronisation
    sfnt[f].data = mib_buf_alloc((size_t)plans[f].sfnt_len);
    if (!sfnt[f].data) {
      use.rc = MIB_E_OUT_OF_MEMORY;
      break;
    }
    sfnt[f].size = (size_t)plans[f].sfnt_len;
    hipMemcpyAsync(sfnt[f].data, d_out + host.fonts[f].out_base, sfnt[f].size, hipMemcpyDeviceToHost, use.st);
  }
  if (hipStreamSynchronize(use.st) != hipSuccess && !use.rc) use.rc = MIB_E_NO_DEVICE;
  if (use.rc)
    for (size_t f = 0; f < k; f++) drop(&sfnt[f]);
  use.timed = use.rc == 0;
  return use.rc;
}

extern "C" int mib_debug_ttc_assemble(uint32_t version, const uint32_t *tags, const mib_span *tables,
                                      const uint8_t *d_src_misalign, size_t k, const uint32_t *font_flavors,
                                      const uint32_t *font_counts, const uint32_t *font_indices, size_t n_fonts, mib_buf *ttc) {
  if (!ttc) return MIB_E_INVALID_ARG;
  ttc->data = nullptr;
  ttc->size = 0;
  if (!tags || !tables || !font_flavors || !font_counts || !font_indices) return MIB_E_INVALID_ARG;
  Plan pl;
  if (!plan_of_collection(version, tags, tables, d_src_misalign, k, font_flavors, font_counts, font_indices, n_fonts, &pl))
    return MIB_E_INVALID_ARG;
  const size_t total = (size_t)pl.stream_len;
  std::vector<uint8_t> stage(total);
  for (size_t i = 0; i < k; i++)
    if (tables[i].size) memcpy(stage.data() + pl.t[i].src_off, tables[i].data, tables[i].size);
  Launch host;   // (declared before the scope: the launches read it until the stream is synchronised)
  Call use(true);
  if (!use.c) return MIB_E_NO_DEVICE;
  uint8_t *d_src = use.m.take<uint8_t>(total), *d_out = nullptr;
  if (!d_src) return use.rc = MIB_E_OUT_OF_MEMORY;
  if (total && hipMemcpyAsync(d_src, stage.data(), total, hipMemcpyHostToDevice, use.st) != hipSuccess)
    return use.rc = MIB_E_NO_DEVICE;
  if (!add_font(&host, pl, FontSrc{d_src, nullptr, nullptr, nullptr})) return use.rc = MIB_E_INVALID_ARG;
  if ((use.rc = assemble_device(use.st, use.tm, use.m, host, &d_out))) return use.rc;
  use.rc = use.fetch(d_out + host.fonts[0].out_base, (size_t)pl.sfnt_len, ttc);
  use.timed = use.rc == 0;
  return use.rc;
}

extern "C" int mib_debug_sfnt_assemble(uint32_t flavor, const uint32_t *tags, const mib_span *tables,
                                       const uint8_t *d_src_misalign, size_t k, mib_buf *sfnt) {
  if (!sfnt) return MIB_E_INVALID_ARG;
  sfnt->data = nullptr;
  sfnt->size = 0;
  if (k == 0 || k > 65535 || !tags || !tables) return MIB_E_INVALID_ARG;   // (k counts tables here: none is no font)
  const uint32_t count = (uint32_t)k;
  return mib_debug_sfnt_assemble_batch(&flavor, &count, tags, tables, d_src_misalign, 1, sfnt);
}
