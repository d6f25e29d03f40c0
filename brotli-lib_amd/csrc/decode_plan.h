// Host planning of a one-shot decode: what runtime.cpp works out from a stream's bytes before it
// touches the device -- window bits, the announced size, the part index (parts.h), the layout of a
// host batch.  Plain C++17, no HIP: the streams are untrusted, so tests/decode_plan_host_main.cpp
// runs this header under AddressSanitizer and UBSan, without a GPU.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/brotli_amd.h"   // mib_span, MIB_IN_PLACE_SLACK, MIB_E_OUTPUT_LIMIT
#include "parts.h"

namespace mib {

// ---------------------------------------------------------------- window bits, announced size
// decodeWindowBits (engine.ts:91-124) on a reader with get(bits): the window's log2 (10..24) and
// the bits read; kLargeWindow for the large-window escape, whose size follows in further bits.
constexpr int kLargeWindow = -1;
struct WindowBits { int lgwin, nbits; };
template <class Bits>
WindowBits read_window_bits(Bits &r) {
  if (r.get(1) == 0) return {16, 1};
  int m = (int)r.get(3);
  if (m) return {17 + m, 4};
  m = (int)r.get(3);
  if (m == 1) return {kLargeWindow, 7};
  return {m ? 8 + m : 17, 7};
}

// LSB-first bit reader over b[0, n): zeros past the end
struct PadBits {
  const uint8_t *b;
  size_t n;
  size_t bit = 0;
  uint32_t get(int k) {
    uint32_t v = 0;
    for (int i = 0; i < k; i++, bit++) {
      const uint32_t byte = (bit >> 3) < n ? b[bit >> 3] : 0;
      v |= ((byte >> (bit & 7)) & 1) << i;
    }
    return v;
  }
};

// the window bits of a stream's first bytes: sizes the ring scratch
inline int peek_window_bits(const uint8_t *b, size_t n) {
  PadBits r{b, n};
  const int lg = read_window_bits(r).lgwin;
  return lg == kLargeWindow ? 24 : lg;   // large window: rejected by the decoder, any ring size will do
}

// mib_decoded_size: engine.ts:2155-2192 (header parse only)
inline int64_t decoded_size(const uint8_t *b, size_t n) {
  PadBits r{b, n};
  if (read_window_bits(r).lgwin == kLargeWindow) {
    if (r.get(1)) return -1;
    r.get(6);
  }
  const int last = (int)r.get(1);
  if (last && r.get(1)) return 0;
  const int nib = (int)r.get(2) + 4;
  if (nib == 7) return -1;
  int64_t mlen = 0;
  for (int i = 0; i < nib; i++) mlen |= (int64_t)r.get(4) << (i * 4);
  return last ? mlen + 1 : -1;
}

// ---------------------------------------------------------------- part index (parts.h)
// A stream's part plan: every valid entry of its index chain, in stream order.
struct PartPlan {
  std::vector<PartEntry> ent;
  int64_t total = -1;
  int lgwin = 0;
};

// LSB-first bit reader over bytes fetched on demand (host memory or the device)
template <class Fetch>
struct HdrBits {
  Fetch &fetch;
  uint64_t bit;
  bool ok = true;
  uint32_t get(int n) {
    uint32_t v = 0;
    for (int i = 0; i < n; i++, bit++) {
      int byte = 0;
      if (!fetch(bit >> 3, 1, (uint8_t *)&byte)) {
        ok = false;
        return 0;
      }
      v |= (uint32_t)((byte >> (bit & 7)) & 1) << i;
    }
    return v;
  }
};

// The index block at byte `at` (with the stream's window bits first when at == 0).
// fetch(offset, length, dst) copies stream bytes; false past the end.
// *end: the byte after the block's payload (where the decoder reads the next header).
template <class Fetch>
bool read_part_index(Fetch &fetch, uint64_t at, PartPlan &plan, uint64_t *next, uint64_t *end) {
  HdrBits<Fetch> r{fetch, at * 8};
  if (at == 0) {
    plan.lgwin = read_window_bits(r).lgwin;
    if (plan.lgwin == kLargeWindow) return false;
  }
  if (r.get(1) != 0 || r.get(2) != 3 || r.get(1) != 0) return false;   // ISLAST 0, metadata, reserved 0
  const int nb = (int)r.get(2);
  if (nb == 0) return false;
  const uint64_t len = (uint64_t)r.get(8 * nb) + 1;
  if (!r.ok || len < sizeof(PartHead)) return false;
  const uint64_t pay = (r.bit + 7) >> 3;
  PartHead h;
  if (!fetch(pay, sizeof(h), (uint8_t *)&h)) return false;
  if (h.magic != kPartMagic || h.version != 1 || h.entry_bytes != sizeof(PartEntry)) return false;
  if (sizeof(h) + (uint64_t)h.nentries * sizeof(PartEntry) > len || h.nentries == 0 || h.nentries > (1u << 20)) return false;
  if (at == 0 && (int)h.lgwin != plan.lgwin) return false;
  std::vector<PartEntry> e(h.nentries);
  if (!fetch(pay + sizeof(h), sizeof(PartEntry) * e.size(), (uint8_t *)e.data())) return false;
  for (auto &x : e)
    if (x.flags & kPartValid) plan.ent.push_back(x);
  plan.total = (int64_t)h.total;
  *next = h.next_byte;
  *end = pay + len;
  return true;
}

// The whole chain of a stream of n bytes; false if it has none or it does not hold together.
// Every part proves it ended exactly at the next entry's state, so the chain of parts is the
// serial decode once its FIRST entry is: that entry must be the metablock header the
// reference decoder reads right after skipping the first index block (its payload is opaque
// to every decoder, so an entry pointing into it -- or anywhere else -- is not trusted).
template <class Fetch>
bool plan_parts(Fetch &fetch, uint64_t n, PartPlan &plan) {
  uint64_t at = 0, next = 0, end = 0, first_end = 0;
  for (int guard = 0; guard < (1 << 16); guard++) {
    if (!read_part_index(fetch, at, plan, &next, &end)) {
      if (at == 0) return false;
      // BrotliEncoder.finish() with nothing pending adds only the final empty metablock
      // (ISLAST, ISLASTEMPTY: one byte 0x03): the chain is complete
      uint8_t b = 0;
      if (n - at == 1 && fetch(at, 1, &b) && b == 0x03) next = 0;
      break;
    }
    if (at == 0) first_end = end;
    if (next == 0) break;
    if (next <= at || next >= n) return false;
    at = next;
  }
  if (next != 0) return false;   // the stream's total is only known from the final chunk's head
  if (plan.ent.size() < 2 || plan.total <= 0 || plan.total > (1ll << 30)) return false;
  if (plan.ent[0].pos != 0 || !(plan.ent[0].flags & kPartAtMb)) return false;
  if (plan.ent[0].bit != 8 * first_end || plan.ent[0].mb_bit != plan.ent[0].bit || plan.ent[0].mb_pos != 0) return false;
  for (size_t i = 0; i < plan.ent.size(); i++) {
    const PartEntry &x = plan.ent[i];
    if (x.bit >= 8 * n || x.mb_bit > x.bit || x.mb_pos > x.pos || x.pos >= (uint64_t)plan.total) return false;
    if (i && (x.pos <= plan.ent[i - 1].pos || x.bit <= plan.ent[i - 1].bit)) return false;
  }
  return true;
}

struct HostFetch {   // stream bytes in host memory
  const uint8_t *b;
  uint64_t n;
  bool operator()(uint64_t off, uint64_t len, uint8_t *dst) const {
    if (off > n || len > n - off) return false;
    memcpy(dst, b + off, len);
    return true;
  }
};
// The first 16 bytes of a stream: window bits then an index block with our magic?
inline bool looks_indexed(const uint8_t *head, uint64_t n) {
  HostFetch f{head, n < 16 ? n : 16};
  HdrBits<HostFetch> r{f, 0};
  if (read_window_bits(r).lgwin == kLargeWindow) return false;
  if (r.get(1) != 0 || r.get(2) != 3 || r.get(1) != 0) return false;
  const int nb = (int)r.get(2);
  if (nb == 0) return false;
  r.get(8 * nb);
  const uint64_t pay = (r.bit + 7) >> 3;
  uint32_t magic = 0;
  return r.ok && f(pay, 4, (uint8_t *)&magic) && magic == kPartMagic;
}

// ---------------------------------------------------------------- output slots of a batch
// What a stream may write when nothing but its header is known: the size the header announces
// (est > 0), else 8x the input and at least 64 KiB.  One that outgrows it is decoded again alone.
inline uint64_t decode_cap(int64_t est, uint64_t in_size) {
  return est > 0 ? (uint64_t)est : 8 * in_size > (1u << 16) ? 8 * in_size : (1u << 16);
}
// A capacity's slot in the host batch's output buffer: + the slack that lets a one-metablock
// stream decode in its slot, + the 64 bytes behind every slot (the job's out_cap is the slot
// less those 64), to a 256-byte boundary.
inline uint64_t decode_slot(uint64_t cap) { return (cap + MIB_IN_PLACE_SLACK + 64 + 255) & ~(uint64_t)255; }

// An announced size above this goes alone under the alone rules (plan_batch)
constexpr int64_t kBatchSlotMax = 64ll << 20;

// kInLaunch: decoded in the batch's one launch, at in_off / out_off; kAlone: by itself once the staging
// buffers are free; kSettled: MIB_E_OUTPUT_LIMIT with the announced size, before any decoding
enum BatchHow : uint8_t { kInLaunch = 0, kAlone = 1, kSettled = 2 };
struct BatchItem {
  BatchHow how;
  int64_t est;                          // decoded_size of the stream
  uint64_t in_off, out_off, out_slot;   // kInLaunch: where its input and output lie, the output slot's bytes
};
struct BatchLayout {
  std::vector<BatchItem> item;
  uint64_t in_bytes = 0, out_bytes = 0;   // the two staging buffers (inputs padded to 256 each)
};

// The layout of mib_decode_batch (alone_rules false, max_out -1) and mib_decode_batch_dictionary
// (alone_rules true).  max_out >= 0: a stream announcing more is settled here (mib_decode: the
// header's size, before decoding).  alone_rules: a stream with a part index goes alone, and so
// does one whose header -- untrusted -- announces more than kBatchSlotMax, so that one stream's
// claim cannot make the shared buffers' allocation, and with it the whole call, fail: alone, a
// failed allocation is that stream's code.
inline BatchLayout plan_batch(const mib_span *in, size_t k, int64_t max_out, bool alone_rules) {
  BatchLayout l;
  l.item.resize(k);
  for (size_t i = 0; i < k; i++) {
    BatchItem &t = l.item[i];
    t = BatchItem{kInLaunch, decoded_size(in[i].data, in[i].size), l.in_bytes, l.out_bytes, 0};
    if (max_out >= 0 && t.est > 0 && t.est > max_out) {
      t.how = kSettled;
    } else if (alone_rules && ((in[i].size >= 16 && looks_indexed(in[i].data, in[i].size)) || t.est > kBatchSlotMax)) {
      t.how = kAlone;
    } else {
      t.out_slot = decode_slot(decode_cap(t.est, in[i].size));
      l.in_bytes += (in[i].size + 255) & ~(uint64_t)255;
      l.out_bytes += t.out_slot;
    }
  }
  return l;
}

}  // namespace mib
