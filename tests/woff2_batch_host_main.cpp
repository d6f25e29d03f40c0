// Stand-alone host build of the WOFF2 batch plan (brotli-lib_amd/csrc/woff2_batch.h), meant to
// be built with -fsanitize=address,undefined (tests/test_woff2_batch_host.py).
//
//   woff2_batch_host plan IN OUT BUDGET   IN: pairs of records (file, decompressed stream), the
//                                         files of one call in its order; BUDGET: the group
//                                         budget in bytes (0: the default).  The call is planned
//                                         as the device path plans it -- groups, stream slots,
//                                         the assembly launch of every group -- with
//                                         host_assemble as the per-font worker and host_run in
//                                         the kernels' place.  OUT gets a pair per input: the
//                                         slot's code (4 bytes, little-endian, two's complement)
//                                         and its sfnt, cut from the group's output buffer.
// Exits non-zero where the plan breaks one of the invariants below.  A record is a u32
// little-endian length + bytes.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "woff2_batch.h"

using namespace mib::woff2file;
typedef std::vector<uint8_t> Bytes;

static std::vector<Bytes> read_records(const char *path) {
  std::vector<Bytes> r;
  FILE *f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", path);
    exit(2);
  }
  uint8_t h[4];
  while (fread(h, 1, 4, f) == 4) {
    const uint32_t n = h[0] | (h[1] << 8) | (h[2] << 16) | ((uint32_t)h[3] << 24);
    Bytes b(n);
    if (n && fread(b.data(), 1, n, f) != n) {
      fprintf(stderr, "short record in %s\n", path);
      exit(2);
    }
    r.push_back(b);
  }
  fclose(f);
  return r;
}
static void write_record(FILE *f, const uint8_t *p, size_t n) {
  const uint8_t h[4] = {(uint8_t)n, (uint8_t)(n >> 8), (uint8_t)(n >> 16), (uint8_t)(n >> 24)};
  fwrite(h, 1, 4, f);
  if (n) fwrite(p, 1, n, f);
}

static void fail(const char *what) {
  fprintf(stderr, "invariant broken: %s\n", what);
  exit(1);
}

// a heap block of exactly n bytes: a read past it is a sanitizer report
static uint8_t *exact(const uint8_t *p, size_t n) {
  uint8_t *q = (uint8_t *)malloc(n ? n : 1);
  if (n) memcpy(q, p, n);
  return q;
}

struct Font {
  size_t slot;   // in the call
  Plan laid;
  Bytes solo;    // host_assemble's sfnt
  uint8_t *glyf, *loca, *hmtx;
  uint64_t base;
  uint32_t first_desc;
};

// The groups keep the files' order, cover every parsed file once, hold at most the budget unless
// they are one file, and are cut no earlier than they must be.
static void check_groups(const std::vector<Group> &groups, const std::vector<uint64_t> &lens, uint64_t budget) {
  if (!budget) budget = kGroupBytes;
  size_t at = 0;
  uint64_t before = 0;
  for (size_t g = 0; g < groups.size(); g++) {
    if (groups[g].first != at || groups[g].count == 0) fail("groups do not follow each other");
    uint64_t sum = 0;
    for (size_t i = 0; i < groups[g].count; i++) sum += lens[at + i];
    if (sum > budget && groups[g].count != 1) fail("a group above the budget holds more than one file");
    if (g && before <= budget && lens[at] <= budget && before + lens[at] <= budget) fail("a group was cut early");
    before = sum;
    at += groups[g].count;
  }
  if (at != lens.size()) fail("groups do not cover the parsed files");
}

static const uint8_t kFill = 0xA5;

int main(int argc, char **argv) {
  if (argc < 5 || std::string(argv[1]) != "plan") return 2;
  const std::vector<Bytes> rec = read_records(argv[2]);
  if (rec.size() % 2) return 2;
  const uint64_t budget = strtoull(argv[4], nullptr, 10);
  const size_t k = rec.size() / 2;
  std::vector<Plan> plans(k);
  std::vector<int> status(k, 0);
  std::vector<Bytes> result(k);
  std::vector<size_t> parsed;
  std::vector<uint64_t> lens;
  for (size_t i = 0; i < k; i++) {
    const Bytes &file = rec[2 * i];
    uint8_t *f = exact(file.data(), file.size());
    status[i] = parse(file.empty() ? nullptr : f, file.size(), &plans[i]) ? 0 : -1;
    free(f);
    if (status[i]) continue;
    parsed.push_back(i);
    lens.push_back(plans[i].stream_len);
  }
  const std::vector<Group> groups = make_groups(lens, budget);
  check_groups(groups, lens, budget);
  size_t fonts_done = 0;
  for (const Group &g : groups) {
    const size_t n = g.count;
    const size_t *idx = &parsed[g.first];
    std::vector<const Plan *> pp(n);
    for (size_t i = 0; i < n; i++) pp[i] = &plans[idx[i]];
    const StreamPack pack = pack_streams(pp.data(), n);
    if (pack.in_off.size() != n + 1 || pack.slot_off.size() != n || pack.cap.size() != n) fail("pack sizes");
    uint64_t end = 0;
    for (size_t i = 0; i < n; i++) {
      if (pack.in_off[i + 1] - pack.in_off[i] != pp[i]->comp_len || (i == 0 && pack.in_off[0] != 0))
        fail("compressed streams are not back to back");
      if (pack.slot_off[i] % kSlotAlign) fail("a stream slot is not at a 256-byte boundary");
      if (pack.slot_off[i] < end) fail("stream slots overlap");
      if (pack.cap[i] != pp[i]->stream_len) fail("a stream's capacity is not its stream_len");
      end = pack.slot_off[i] + pack.cap[i];
      if (end > pack.stream_bytes) fail("a stream slot leaves the buffer");
    }
    uint8_t *streams = (uint8_t *)malloc(pack.stream_bytes ? pack.stream_bytes : 1);
    memset(streams, kFill, pack.stream_bytes);
    std::vector<Font> fonts;
    Launch launch;
    for (size_t i = 0; i < n; i++) {
      const Bytes &file = rec[2 * idx[i]], &stream = rec[2 * idx[i] + 1];
      if (stream.size() != pp[i]->stream_len) {   // (what a stream of another size is to the device path)
        status[idx[i]] = -1;
        continue;
      }
      if (!stream.empty()) memcpy(streams + pack.slot_off[i], stream.data(), stream.size());
      Font f;
      f.slot = idx[i];
      f.glyf = f.loca = f.hmtx = nullptr;
      if (host_assemble(file.data(), file.size(), stream.empty() ? nullptr : stream.data(), stream.size(), &f.solo, &f.laid) != 0) {
        status[idx[i]] = -1;
        continue;
      }
      // the reconstructed tables as the per-font worker left them, each in a block of its own
      for (const Table &t : f.laid.t) {
        uint8_t **where = t.kind == kGlyf ? &f.glyf : t.kind == kLoca ? &f.loca : t.kind == kHmtx ? &f.hmtx : nullptr;
        if (where) *where = exact(f.solo.data() + t.dst_off, t.dst_len);
      }
      f.first_desc = (uint32_t)launch.descs.size();
      if (!add_font(&launch, f.laid, FontSrc{streams + pack.slot_off[i], f.glyf, f.loca, f.hmtx})) fail("add_font refused a font");
      f.base = launch.fonts.back().out_base;
      // sources inside the font's stream, destinations inside the font's range
      const uint8_t *lo = streams + pack.slot_off[i], *hi = lo + pack.cap[i];
      const uint32_t num = (uint32_t)f.laid.t.size();
      if (launch.descs.size() != (size_t)f.first_desc + num || launch.recs.size() != launch.descs.size()) fail("descriptor count");
      for (uint32_t q = 0; q < num; q++) {
        const AsmDesc &d = launch.descs[f.first_desc + q];
        const Table &t = f.laid.t[q];
        if (d.out_base != f.base || d.sum != f.first_desc + q) fail("a descriptor's base or sum slot");
        if (t.kind == kCopy && (d.src < lo || d.src + d.len > hi)) fail("a descriptor's source leaves its font's stream");
        const uint64_t padded = ((uint64_t)d.len + 3) & ~3ull;
        if ((d.dst_off & 3) || d.dst_off < 12 + 16 * (uint64_t)num || d.dst_off + padded > f.laid.sfnt_len)
          fail("a descriptor's destination leaves its font's range");
        if (d.zero_at != kNoZero && (d.zero_at != 8 || d.len < 12)) fail("zero_at");
      }
      const DirFont &df = launch.fonts.back();
      if (df.first_rec != f.first_desc || df.first_sum != f.first_desc || df.num != num) fail("a font's first record or sum");
      for (uint32_t r = 0; r < num; r++)
        if (launch.recs[df.first_rec + r].table >= num) fail("a record's table leaves its font");
      if (df.adjust_at != kNoZero && (uint64_t)df.adjust_at + 4 > f.laid.sfnt_len) fail("adjust_at leaves its font");
      fonts.push_back(std::move(f));
    }
    // sfnt ranges: at 16-byte boundaries, ascending, apart, inside the buffer
    uint64_t at = 0;
    for (const Font &f : fonts) {
      if (f.base % kFontAlign) fail("an sfnt is not at a 16-byte boundary");
      if (f.base < at) fail("sfnt ranges overlap");
      at = f.base + f.laid.sfnt_len;
      if (at > launch.out_bytes) fail("an sfnt leaves the output buffer");
    }
    if (at != launch.out_bytes) fail("the output buffer is not the last sfnt's end");
    uint8_t *out = (uint8_t *)malloc(launch.out_bytes ? launch.out_bytes : 1);
    memset(out, kFill, launch.out_bytes);
    host_run(launch, out);
    at = 0;
    for (const Font &f : fonts) {
      for (uint64_t b = at; b < f.base; b++)
        if (out[b] != kFill) fail("a byte between two fonts was written");
      if (f.solo.size() != f.laid.sfnt_len || memcmp(out + f.base, f.solo.data(), f.solo.size()) != 0)
        fail("the batch's sfnt is not the per-font worker's");
      result[f.slot].assign(out + f.base, out + f.base + f.laid.sfnt_len);
      at = f.base + f.laid.sfnt_len;
      free(f.glyf);
      free(f.loca);
      free(f.hmtx);
    }
    fonts_done += fonts.size();
    free(out);
    free(streams);
  }
  FILE *o = fopen(argv[3], "wb");
  if (!o) return 2;
  for (size_t i = 0; i < k; i++) {
    const uint32_t u = (uint32_t)status[i];
    const uint8_t c[4] = {(uint8_t)u, (uint8_t)(u >> 8), (uint8_t)(u >> 16), (uint8_t)(u >> 24)};
    write_record(o, c, 4);
    write_record(o, result[i].data(), result[i].size());
  }
  fclose(o);
  printf("files %zu parsed %zu groups %zu fonts %zu\n", k, parsed.size(), groups.size(), fonts_done);
  return 0;
}
