// brotli_amd host runtime: the C ABI of include/brotli_amd.h on top of the HIP kernels.
//
// Host work here is orchestration only -- argument handling mirroring decode.ts / encode.ts,
// header peeks, buffer sizing, H2D/D2H copies.  Every byte of encode/decode compute runs in
// the kernels (decode.hip, encode*.hip); with no gfx950 device the calls fail with
// MIB_E_NO_DEVICE rather than falling back to the CPU.
// What a one-shot decode works out from a stream's bytes alone (window bits, announced size, the
// part index reader plan_parts, a host batch's slots) is decode_plan.h, which host tests run under
// sanitizers; here: decode_jobs / decode_parts (a launch each), decode_one and decode_batch over them.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <chrono>
#include <functional>
#include <memory>
#include <thread>
#include <vector>

#include "common.h"
#include "decode_plan.h"
#include "dictionary.h"
#include "parts.h"
#include "stream_session.h"
#include "stream_batch.h"
#include "stream_rounds.h"

// (d_heads: one checkpoint head per job, loaded before and stored after the job runs)
extern "C" hipError_t mib_decode_resume_launch(mib::StreamJob *d_jobs, int njobs, uint8_t *d_scratch, uint64_t per_block,
                                               int grid, int per_cu, uint8_t *d_heads, hipStream_t stream);
extern "C" hipError_t mib_stream_move_batch_launch(const mib::MoveDesc *d_descs, const mib::MoveUnit *d_units, uint32_t n_units,
                                                   hipStream_t stream);
extern "C" hipError_t mib_stream_copy_batch_launch(const mib::CopyDesc *d_descs, uint32_t k, uint32_t blocks, hipStream_t stream);
extern "C" hipError_t mib_decode_stream_init_tables(const int16_t *host_lut);
extern "C" hipError_t mib_decode_parts_launch(mib::DecJob *d_jobs, int njobs, uint8_t *d_scratch, uint64_t per_block,
                                              unsigned *d_ticket, int grid, int per_cu, hipStream_t stream);
extern "C" hipError_t mib_decode_launch(mib::DecJob *d_jobs, int njobs, uint8_t *d_scratch, uint64_t per_block,
                                        uint64_t ring_bytes, int grid, int per_cu, hipStream_t stream);
extern "C" hipError_t mib_decode_init_tables(const int16_t *host_lut);
extern "C" hipError_t mib_decode_peek_heads(const uint8_t *d_in, const uint64_t *d_offsets, int k, uint8_t *d_heads,
                                            hipStream_t stream);

const char *mib::knob(const char *name) {
#ifdef MIB_EXPERIMENTS
  return getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}

namespace {
bool g_dev_unordered_any(int dev);
}
bool mib::lds_rank_ordered(int dev) { return !g_dev_unordered_any(dev); }

namespace {

#define HIP_OK(x)                               \
  do {                                          \
    hipError_t e_ = (x);                        \
    if (e_ != hipSuccess) return MIB_E_NO_DEVICE; \
  } while (0)

std::mutex g_mu;
int g_device = 0;                 // device of the default context (mib_init)
constexpr int kMaxDevices = 64;
bool g_dev_ready[kMaxDevices];    // per device: checked to be gfx950, command table uploaded
bool g_dev_unordered[kMaxDevices];  // per device: the LDS atomic order self-test failed
int g_dev_cus[kMaxDevices];       // per device: compute units

void build_cmd_lut(int16_t *lut) {   // engine.ts:65-90
  static const int ins_bits[24] = {0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7, 8, 9, 10, 12, 14, 24};
  static const int copy_bits[24] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 7, 8, 9, 10, 24};
  int ins_off[24], copy_off[24];
  ins_off[0] = 0;
  copy_off[0] = 2;
  for (int i = 0; i < 23; i++) {
    ins_off[i + 1] = ins_off[i] + (1 << ins_bits[i]);
    copy_off[i + 1] = copy_off[i] + (1 << copy_bits[i]);
  }
  for (int c = 0; c < 704; c++) {
    int r = c >> 6, dco = -4;
    if (r >= 2) {
      r -= 2;
      dco = 0;
    }
    int ic = (((0x29850 >> (r * 2)) & 3) << 3) | ((c >> 3) & 7);
    int cc = (((0x26244 >> (r * 2)) & 3) << 3) | (c & 7);
    int co = copy_off[cc];
    lut[4 * c] = (int16_t)(ins_bits[ic] | (copy_bits[cc] << 8));
    lut[4 * c + 1] = (int16_t)ins_off[ic];
    lut[4 * c + 2] = (int16_t)co;
    lut[4 * c + 3] = (int16_t)(dco + std::min(co, 5) - 2);
  }
}

// Every device a context runs on is checked (gfx950) and gets its own copy of the decoder's
// __constant__ command table: module globals are per device.  Leaves `device` current.
int g_ndev = -1;   // visible devices, counted once (hipGetDeviceCount cost ~0.4 ms a call, r05m)
int ensure_device(int device) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (g_ndev <= 0) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return MIB_E_NO_DEVICE;
    g_ndev = n;
  }
  if (device < 0 || device >= g_ndev || device >= kMaxDevices) return MIB_E_NO_DEVICE;
  HIP_OK(hipSetDevice(device));
  if (g_dev_ready[device]) return 0;
  hipDeviceProp_t prop;
  HIP_OK(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    fprintf(stderr, "brotli_amd: device %d is %s, this build targets gfx950\n", device, prop.gcnArchName);
    return MIB_E_NO_DEVICE;
  }
  g_dev_cus[device] = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  int16_t lut[704 * 4];
  build_cmd_lut(lut);
  HIP_OK(mib_decode_init_tables(lut));
  HIP_OK(mib_decode_stream_init_tables(lut));
  HIP_OK(hipDeviceSynchronize());
  const int64_t bad = mib_selftest_lds_atomic_order(4096);
  if (bad < 0) return MIB_E_NO_DEVICE;
  g_dev_unordered[device] = bad != 0;
  if (bad)
    fprintf(stderr, "brotli_amd: device %d serves returning LDS atomics out of lane order (%lld of 262144 lanes); "
                    "the bucket sort ranks by ballots\n", device, (long long)bad);
  g_dev_ready[device] = true;
  return 0;
}

int g_force_ballot = 0;
bool g_dev_unordered_any(int dev) {
  return __atomic_load_n(&g_force_ballot, __ATOMIC_RELAXED) || (dev >= 0 && dev < kMaxDevices && g_dev_unordered[dev]);
}

int ensure_init() {
  int dev;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    dev = g_device;
  }
  return ensure_device(dev);
}

struct DeviceFetch {   // plan_parts' stream bytes on the device (small reads: index heads and entries)
  const uint8_t *d;
  uint64_t n;
  hipStream_t st;
  uint64_t cache_off = ~0ull;
  uint8_t cache[64] = {};
  bool operator()(uint64_t off, uint64_t len, uint8_t *dst) {
    if (off > n || len > n - off) return false;
    if (len == 1) {   // header bits: one cached 64-byte line at a time
      if (cache_off == ~0ull || off < cache_off || off >= cache_off + 64) {
        cache_off = off & ~63ull;
        const uint64_t m = std::min<uint64_t>(64, n - cache_off);
        if (hipMemcpyAsync(cache, d + cache_off, m, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
          return false;
      }
      *dst = cache[off - cache_off];
      return true;
    }
    return hipMemcpyAsync(dst, d + off, len, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
  }
};

// Waves a decode launch puts on each CU (1..4): a call with few streams gives each stream
// a whole CU's LDS (decode.hip decode_lds_plan)
int waves_per_cu(int device, size_t waves) {
  const size_t cus = (device >= 0 && device < kMaxDevices && g_dev_cus[device] > 0) ? (size_t)g_dev_cus[device] : 256;
  const size_t w = (waves + cus - 1) / cus;
  return (int)std::max<size_t>(1, std::min<size_t>(4, w));
}

}  // namespace

constexpr int kEncLanes = 4;                  // encode lanes at most (encode.hip)
constexpr int kStageSlots = 4 + kEncLanes - 1;   // + lanes 1.. packed output
struct mib_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  // decode scratch
  uint8_t *d_scratch = nullptr;
  uint64_t scratch_bytes = 0;
  mib::DecJob *d_jobs = nullptr;
  size_t jobs_cap = 0;
  uint8_t *d_aux = nullptr;   // small per-call staging (offsets, header peeks)
  uint64_t aux_bytes = 0;
  // part decoding: entries, positions, progress words, ticket (one allocation)
  uint8_t *d_parts = nullptr;
  uint64_t parts_bytes = 0;
  // batches of decoder sessions (mib_decoder_update_batch): a round's jobs, checkpoint heads and
  // move / copy descriptors, and the staging span a host call's output is copied into
  uint8_t *d_sbatch = nullptr;
  uint64_t sbatch_bytes = 0;
  uint8_t *d_sspan = nullptr;
  uint64_t sspan_bytes = 0;
  // encode workspaces (encode.hip): lane 0 on `stream`, lane l > 0 on lane_stream[l] (a batch
  // encode runs as concurrent parts, encode_streams)
  void *enc_ws = nullptr;
  void *lane_ws[kEncLanes] = {};
  hipStream_t lane_stream[kEncLanes] = {};
  // staging buffers of the host-memory entry points (input, output, dictionary, encoder
  // output) and lane 1's packed output, kept across calls so a small call does not pay
  // hipMalloc / hipFree
  uint8_t *stage[kStageSlots] = {};
  uint64_t stage_cap[kStageSlots] = {};
  // what the calls since the last trim needed of each buffer (trim's hysteresis, below)
  struct Trim {
    uint64_t need = 0;
    int quiet = 0;   // trims in a row whose calls needed no more than the keep size
  } stage_trim[kStageSlots], scratch_trim, parts_trim, sspan_trim;
  // pinned host ring of the host <-> device transfers (host_io below): two halves, one filling
  // on the host while the other is in flight; allocated once, 2 x kRingHalf
  uint8_t *ring = nullptr;
  hipEvent_t ring_ev[2] = {nullptr, nullptr};
  bool ring_failed = false;
  // part decoding counters (streams decoded part-parallel / sent back to the serial decoder)
  uint64_t parts_used = 0, parts_fallback = 0;
  // the last serial decode launch: streams that finished in their output slots / left them part-way
  uint64_t in_place_done = 0, in_place_left = 0;
  // profiling
  int profiling = 0;   // 0 off, 1 every kernel, 2 the decoder's only (mib_ctx_set_profiling)
  std::vector<mib_kernel_time> times;
  std::mutex times_mu;   // (two encode lanes collect at once)
  void add_time(const char *name, double ms) {
    std::lock_guard<std::mutex> lk(times_mu);
    for (auto &t : times)
      if (strncmp(t.name, name, sizeof(t.name)) == 0) {
        t.ms += ms;
        t.launches++;
        return;
      }
    mib_kernel_time t;
    memset(&t, 0, sizeof(t));
    strncpy(t.name, name, sizeof(t.name) - 1);
    t.ms = ms;
    t.launches = 1;
    times.push_back(t);
  }
};

extern "C" void mib_ctx_add_time(mib_ctx *c, const char *name, double ms) { c->add_time(name, ms); }
extern "C" int mib_ctx_profiling(mib_ctx *c) { return c->profiling; }
extern "C" void **mib_ctx_enc_ws(mib_ctx *c) { return &c->enc_ws; }
// encode lane l (1 .. kEncLanes - 1): its workspace slot, its stream (created on first use, on
// the context's device)
extern "C" void **mib_ctx_lane_ws(mib_ctx *c, int l) { return &c->lane_ws[l]; }
extern "C" void *mib_ctx_lane_stream(mib_ctx *c, int l) {
  if (!c->lane_stream[l]) {
    hipSetDevice(c->device);
    if (hipStreamCreateWithFlags(&c->lane_stream[l], hipStreamNonBlocking) != hipSuccess) c->lane_stream[l] = nullptr;
  }
  return (void *)c->lane_stream[l];
}
int grow(void **p, uint64_t *cap, uint64_t need);
// a staging buffer of at least `need` bytes (its content is not kept when it grows)
extern "C" uint8_t *mib_ctx_stage(mib_ctx *c, int slot, uint64_t need) {
  if (slot < 0 || slot >= kStageSlots) return nullptr;
  c->stage_trim[slot].need = std::max(c->stage_trim[slot].need, need);
  return grow((void **)&c->stage[slot], &c->stage_cap[slot], need) == 0 ? c->stage[slot] : nullptr;
}
extern "C" void mib_encode_ws_free(void *ws);

// ---------------------------------------------------------------- host <-> device transfers
// Host buffers cross PCIe through the context's pinned ring: the host copies a ring half while
// the other half is in flight, and host copies of more than a few MiB run on several threads.
// Pageable hipMemcpy of many 1 MiB results into fresh host memory ran at 0.5-2 GB/s and varied
// by 8x between runs; pinned halves move at PCIe speed, and the page faults
// of fresh result buffers are spread over the copy threads.
namespace {
constexpr uint64_t kRingHalf = 32ull << 20;
constexpr uint64_t kParCopyMin = 4ull << 20;   // below this, one thread copies
constexpr int kCopyThreads = 8;
using Piece = mib::HostPiece;
void par_copy(const std::vector<Piece> &ps) {
  uint64_t total = 0;
  for (const Piece &p : ps) total += p.n;
  const int nt = (int)std::min<uint64_t>(kCopyThreads, std::max<uint64_t>(1, total / kParCopyMin));
  auto run = [&](uint64_t lo, uint64_t hi) {   // bytes [lo, hi) of the concatenated pieces
    uint64_t at = 0;
    for (const Piece &p : ps) {
      const uint64_t a = std::max(lo, at), b = std::min(hi, at + p.n);
      if (a < b) memcpy(p.dst + (a - at), p.src + (a - at), b - a);
      at += p.n;
      if (at >= hi) break;
    }
  };
  if (nt <= 1) {
    run(0, total);
    return;
  }
  std::vector<std::thread> th;
  for (int t = 1; t < nt; t++) th.emplace_back(run, total * t / nt, total * (t + 1) / nt);
  run(0, total / nt);
  for (auto &x : th) x.join();
}
bool ring_ready(mib_ctx *c) {
  if (c->ring) return true;
  if (c->ring_failed) return false;
  hipSetDevice(c->device);
  if (hipHostMalloc((void **)&c->ring, 2 * kRingHalf, hipHostMallocDefault) != hipSuccess) c->ring = nullptr;
  for (int h = 0; h < 2 && c->ring; h++)
    if (hipEventCreateWithFlags(&c->ring_ev[h], hipEventDisableTiming) != hipSuccess) {
      hipHostFree(c->ring);
      c->ring = nullptr;
    }
  if (!c->ring) c->ring_failed = true;
  return c->ring != nullptr;
}
// the pieces cut at ring-half boundaries: chunk j = the pieces' bytes [j H, (j + 1) H)
template <class F>
void for_chunks(const Piece *ps, size_t k, F fn) {
  std::vector<Piece> cur;
  uint64_t fill = 0;
  for (size_t i = 0; i < k; i++) {
    uint64_t off = 0;
    while (off < ps[i].n) {
      const uint64_t take = std::min(ps[i].n - off, kRingHalf - fill);
      cur.push_back(Piece{ps[i].dst + off, ps[i].src + off, take});
      off += take;
      fill += take;
      if (fill == kRingHalf) {
        fn(cur, fill);
        cur.clear();
        fill = 0;
      }
    }
  }
  if (fill) fn(cur, fill);
}
}  // namespace

// MIB_HOST_TIMING (experiment builds): each ring transfer's time waiting for the device and
// copying on the host, to stderr
namespace {
struct XferClock {
  const bool on = mib::knob("MIB_HOST_TIMING") != nullptr;
  const char *what;
  uint64_t bytes = 0;
  double wait_ms = 0, copy_ms = 0;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  explicit XferClock(const char *w) : what(w) {}
  template <class F>
  void timed(double &acc, F fn) {
    if (!on) return fn();
    const auto a = std::chrono::steady_clock::now();
    fn();
    acc += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
  }
  ~XferClock() {
    if (on)
      fprintf(stderr, "[mib] %s %.1f MiB: %.2f ms (device wait %.2f, host copy %.2f)\n", what, bytes / 1048576.0,
              std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), wait_ms, copy_ms);
  }
};
}  // namespace
// host -> device: ps[i].src host, ps[i].dst device; asynchronous on st (returns once every
// source byte is in the ring: the caller may reuse its buffers)
int mib::ctx_upload(mib_ctx *c, void *stream, const HostPiece *ps, size_t k) {
  hipStream_t st = (hipStream_t)stream;
  uint64_t total = 0;
  for (size_t i = 0; i < k; i++) total += ps[i].n;
  if (total < kParCopyMin || !ring_ready(c)) {   // small: pageable copies
    for (size_t i = 0; i < k; i++)
      if (ps[i].n && hipMemcpyAsync(ps[i].dst, ps[i].src, ps[i].n, hipMemcpyHostToDevice, st) != hipSuccess) return MIB_E_NO_DEVICE;
    return 0;
  }
  int h = 0, rc = 0;
  XferClock clk("upload");
  clk.bytes = total;
  for_chunks(ps, k, [&](const std::vector<Piece> &ch, uint64_t) {
    if (rc) return;
    clk.timed(clk.wait_ms, [&] {   // the half's last copies are done
      if (hipEventSynchronize(c->ring_ev[h]) != hipSuccess) rc = MIB_E_NO_DEVICE;
    });
    if (rc) return;
    uint8_t *pin = c->ring + (uint64_t)h * kRingHalf;
    std::vector<Piece> hc;
    uint64_t po = 0;
    for (const Piece &p : ch) {
      hc.push_back(Piece{pin + po, p.src, p.n});
      po += p.n;
    }
    clk.timed(clk.copy_ms, [&] { par_copy(hc); });
    po = 0;
    for (const Piece &p : ch) {
      if (hipMemcpyAsync(p.dst, pin + po, p.n, hipMemcpyHostToDevice, st) != hipSuccess) { rc = MIB_E_NO_DEVICE; return; }
      po += p.n;
    }
    if (hipEventRecord(c->ring_ev[h], st) != hipSuccess) rc = MIB_E_NO_DEVICE;
    h ^= 1;
  });
  return rc;
}
// device -> host: ps[i].src device (written by work queued on st), ps[i].dst host; returns
// when every byte has arrived
int mib::ctx_download(mib_ctx *c, void *stream, const HostPiece *ps, size_t k) {
  hipStream_t st = (hipStream_t)stream;
  uint64_t total = 0;
  for (size_t i = 0; i < k; i++) total += ps[i].n;
  XferClock clk("download");
  clk.bytes = total;
  if (total < kParCopyMin || !ring_ready(c)) {
    for (size_t i = 0; i < k; i++)
      if (ps[i].n && hipMemcpyAsync(ps[i].dst, ps[i].src, ps[i].n, hipMemcpyDeviceToHost, st) != hipSuccess) return MIB_E_NO_DEVICE;
    return hipStreamSynchronize(st) == hipSuccess ? 0 : MIB_E_NO_DEVICE;
  }
  int h = 0, rc = 0;
  std::vector<Piece> pending;   // the previous chunk: ring -> host once its copies are done
  int ph = 0;
  auto drain = [&]() {
    if (pending.empty() || rc) return;
    clk.timed(clk.wait_ms, [&] {
      if (hipEventSynchronize(c->ring_ev[ph]) != hipSuccess) rc = MIB_E_NO_DEVICE;
    });
    if (rc) return;
    clk.timed(clk.copy_ms, [&] { par_copy(pending); });
    pending.clear();
  };
  for_chunks(ps, k, [&](const std::vector<Piece> &ch, uint64_t) {
    if (rc) return;
    uint8_t *pin = c->ring + (uint64_t)h * kRingHalf;
    std::vector<Piece> out;
    uint64_t po = 0;
    for (const Piece &p : ch) {
      if (hipMemcpyAsync(pin + po, p.src, p.n, hipMemcpyDeviceToHost, st) != hipSuccess) { rc = MIB_E_NO_DEVICE; return; }
      out.push_back(Piece{p.dst, pin + po, p.n});
      po += p.n;
    }
    if (hipEventRecord(c->ring_ev[h], st) != hipSuccess) { rc = MIB_E_NO_DEVICE; return; }
    drain();   // the other half, while this one is in flight
    pending = std::move(out);
    ph = h;
    h ^= 1;
  });
  drain();
  return rc;
}

namespace {

mib_ctx *g_default_ctx = nullptr;
// The host-buffer entry points (mib_encode / mib_decode / batches / BrotliEncoder) share the
// default context's stream and scratch: one call at a time (recursive: a batch decode retries
// a stream through mib_decode).
std::recursive_mutex g_default_mu;

mib_ctx *default_ctx() {
  if (ensure_init() != 0) return nullptr;
  std::lock_guard<std::mutex> lk(g_mu);
  if (!g_default_ctx) {
    g_default_ctx = new mib_ctx();
    g_default_ctx->device = g_device;
    if (hipStreamCreateWithFlags(&g_default_ctx->stream, hipStreamNonBlocking) != hipSuccess) {
      delete g_default_ctx;
      g_default_ctx = nullptr;
    }
  }
  return g_default_ctx;
}

}  // namespace
int grow(void **p, uint64_t *cap, uint64_t need) {
  if (*cap >= need) return 0;
  if (*p) hipFree(*p);
  *p = nullptr;
  *cap = 0;
  uint64_t n = std::max<uint64_t>(need, 1 << 20);
  if (hipMalloc(p, n) != hipSuccess) return MIB_E_OUT_OF_MEMORY;
  *cap = n;
  return 0;
}
extern "C" {

void mib_enc_opts_default(mib_enc_opts *o) {
  o->quality = 11;
  o->lgwin = 22;
  o->mode = MIB_MODE_GENERIC;
  o->size_hint = 0;
  o->dict = nullptr;
  o->dict_len = 0;
  o->stream_chunk = 0;
}

int mib_init(int device) {
  {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_default_ctx && device != g_device) return MIB_E_INVALID_ARG;   // the default context exists already
    g_device = device;
  }
  return ensure_init();
}

const char *mib_strerror(int code) {
  static thread_local char buf[96];
  if (code <= -1 && code >= -30) {
    snprintf(buf, sizeof(buf), "Brotli error code: %d", code);
    return buf;
  }
  switch (code) {
    case 0: return "ok";
    case MIB_E_NO_DEVICE: return "brotli_amd: no usable gfx950 (MI355X) device";
    case MIB_E_INVALID_ARG: return "brotli_amd: invalid argument";
    case MIB_E_OUT_OF_MEMORY: return "brotli_amd: out of device memory";
    case MIB_E_OUTPUT_LIMIT: return "Decompressed size exceeds limit";
    case MIB_E_NEED_SPACE: return "brotli_amd: output buffer too small";
    case MIB_E_JS_RANGE_ERROR: return "RangeError: offset is out of bounds";
    case MIB_E_JS_TYPE_ERROR: return "TypeError: Cannot read property 'subarray' of undefined";
    case MIB_E_NO_PROGRESS: return "brotli_amd: decoder made no progress";
  }
  snprintf(buf, sizeof(buf), "brotli_amd: error %d", code);
  return buf;
}

static mib_alloc_func g_alloc = nullptr;
static mib_free_func g_free = nullptr;
static void *g_opaque = nullptr;

void mib_set_allocator(mib_alloc_func alloc_func, mib_free_func free_func, void *opaque) {
  const bool both = alloc_func && free_func;
  g_alloc = both ? alloc_func : nullptr;
  g_free = both ? free_func : nullptr;
  g_opaque = both ? opaque : nullptr;
}

uint8_t *mib_buf_alloc(size_t n) {
  return (uint8_t *)(g_alloc ? g_alloc(g_opaque, n) : malloc(n ? n : 1));
}

int mib_buf_from_device(mib_buf *out, const void *d_src, uint64_t len) {
  out->data = mib_buf_alloc(len);
  out->size = 0;
  if (!out->data) return MIB_E_OUT_OF_MEMORY;
  out->size = len;
  // (called with the default context held: its stream produced d_src; large results go
  // through its pinned ring)
  mib_ctx *c = default_ctx();
  const mib::HostPiece p{out->data, (const uint8_t *)d_src, len};
  if (len && (!c || mib::ctx_download(c, c->stream, &p, 1) != 0)) {
    mib_buf_free(out);
    return MIB_E_NO_DEVICE;
  }
  return 0;
}

static int bufs_from_device(size_t k, mib_buf *const *outs, const uint8_t *const *d_src, const uint64_t *len);
// On failure no result stays allocated: a caller that reports the error keeps no buffer
// (the Python mirror's allocator would otherwise hold those bytes for the process' life)
int mib_bufs_from_device(size_t k, mib_buf *const *outs, const uint8_t *const *d_src, const uint64_t *len) {
  for (size_t i = 0; i < k; i++) outs[i]->data = nullptr, outs[i]->size = 0;
  const int rc = bufs_from_device(k, outs, d_src, len);
  if (rc)
    for (size_t i = 0; i < k; i++) mib_buf_free(outs[i]);
  return rc;
}
static int bufs_from_device(size_t k, mib_buf *const *outs, const uint8_t *const *d_src, const uint64_t *len) {
  if (!k) return 0;
  const uint8_t *lo = d_src[0], *hi = d_src[0];
  uint64_t sum = 0;
  for (size_t i = 0; i < k; i++) {
    lo = std::min(lo, d_src[i]);
    hi = std::max(hi, d_src[i] + len[i]);
    sum += len[i];
  }
  for (size_t i = 0; i < k; i++) {
    outs[i]->data = mib_buf_alloc(len[i]);
    outs[i]->size = 0;
    if (!outs[i]->data) return MIB_E_OUT_OF_MEMORY;
    outs[i]->size = len[i];
  }
  const uint64_t span = (uint64_t)(hi - lo);
  const bool sparse = span > 4 * sum + (1u << 20);
  // Large results on average (or scattered ones): through the default context's pinned ring,
  // straight into the result buffers, one device copy each.  Many small results in a dense
  // span: the span as ONE device copy (through the ring when large), then host copies out of
  // it -- a device copy call costs ~10 us, thousands of them would dominate.
  if (sparse || sum / k >= (256u << 10)) {
    mib_ctx *c = default_ctx();
    if (!c) return MIB_E_NO_DEVICE;
    std::vector<mib::HostPiece> ps;
    for (size_t i = 0; i < k; i++)
      if (len[i]) ps.push_back(mib::HostPiece{outs[i]->data, d_src[i], len[i]});
    return mib::ctx_download(c, c->stream, ps.data(), ps.size());
  }
  std::vector<uint8_t> host(span);
  if (span >= kParCopyMin) {
    mib_ctx *c = default_ctx();
    if (!c) return MIB_E_NO_DEVICE;
    const mib::HostPiece whole{host.data(), lo, span};
    if (mib::ctx_download(c, c->stream, &whole, 1) != 0) return MIB_E_NO_DEVICE;
  } else if (hipMemcpy(host.data(), lo, span, hipMemcpyDeviceToHost) != hipSuccess) {
    return MIB_E_NO_DEVICE;
  }
  std::vector<Piece> out;
  for (size_t i = 0; i < k; i++)
    if (len[i]) out.push_back(Piece{outs[i]->data, host.data() + (d_src[i] - lo), len[i]});
  par_copy(out);
  return 0;
}

void mib_buf_free(mib_buf *b) {
  if (b && b->data) {
    if (g_free) g_free(g_opaque, b->data);
    else free(b->data);
  }
  if (b) {
    b->data = nullptr;
    b->size = 0;
  }
}

int64_t mib_decoded_size(const uint8_t *b, size_t n) { return mib::decoded_size(b, n); }

mib_ctx *mib_ctx_new(int device) {
  if (ensure_device(device) != 0) return nullptr;
  mib_ctx *c = new mib_ctx();
  c->device = device;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return nullptr;
  }
  return c;
}

void mib_ctx_free(mib_ctx *c) {
  if (!c) return;
  hipSetDevice(c->device);
  if (c->d_scratch) hipFree(c->d_scratch);
  if (c->d_jobs) hipFree(c->d_jobs);
  if (c->d_aux) hipFree(c->d_aux);
  if (c->d_parts) hipFree(c->d_parts);
  if (c->d_sbatch) hipFree(c->d_sbatch);
  if (c->d_sspan) hipFree(c->d_sspan);
  for (int i = 0; i < kStageSlots; i++)
    if (c->stage[i]) hipFree(c->stage[i]);
  if (c->enc_ws) mib_encode_ws_free(c->enc_ws);
  if (c->ring) hipHostFree(c->ring);
  for (int h = 0; h < 2; h++)
    if (c->ring_ev[h]) hipEventDestroy(c->ring_ev[h]);
  if (c->stream) hipStreamDestroy(c->stream);
  for (int l = 0; l < kEncLanes; l++) {
    if (c->lane_ws[l]) mib_encode_ws_free(c->lane_ws[l]);
    if (c->lane_stream[l]) hipStreamDestroy(c->lane_stream[l]);
  }
  delete c;
}

void mib_ctx_set_profiling(mib_ctx *c, int on) { c->profiling = on == 2 ? 2 : on != 0 ? 1 : 0; }

void mib_part_stats(mib_ctx *c, uint64_t *parallel, uint64_t *fallback) {
  if (!c) c = default_ctx();
  if (parallel) *parallel = c ? c->parts_used : 0;
  if (fallback) *fallback = c ? c->parts_fallback : 0;
}

void mib_debug_in_place(mib_ctx *c, uint64_t *finished, uint64_t *left) {
  if (!c) c = default_ctx();
  if (finished) *finished = c ? c->in_place_done : 0;
  if (left) *left = c ? c->in_place_left : 0;
}

// internal (encode.hip)
mib_ctx *mib_default_ctx(void) { return default_ctx(); }
// The host-memory entry points (here, encode.hip, woff2.hip) hold the default context for one
// call at a time; when the outermost of them returns, buffers a large call grew are released:
// a long-lived server keeps what its usual calls need (the latency path stays free of
// hipMalloc), not GiBs reserved since its largest call (a 1 GiB brotliDecode: a 1 GiB input
// stage and a 2 GiB output stage).
constexpr uint64_t kKeepStage = 64ull << 20;      // staging buffers (input, output, dictionary, encoder output)
constexpr uint64_t kKeepScratch = 1ull << 30;     // decoder scratch, part tables, encoder workspace
int g_default_depth = 0;                          // (guarded by g_default_mu)
extern "C" void mib_encode_ws_trim(void **ws, uint64_t keep);
extern "C" int mib_live_encoders(void);
// Hysteresis: a buffer above its keep size is released only once kQuietCalls trims in a row
// saw calls that needed no more than that -- a service whose every call is large keeps its
// buffers (a hipFree syncs the device and a fresh hipMalloc of GiBs costs more than the call:
// the r04 host-batch legs varied by 2 s from it), one large call among
// small ones gives its memory back a few calls later.
constexpr int kQuietCalls = 4;
static void release_large(uint8_t **p, uint64_t *cap, uint64_t keep, mib_ctx::Trim &tr) {
  tr.quiet = tr.need > keep ? 0 : tr.quiet + 1;
  tr.need = 0;
  if (*p && *cap > keep && tr.quiet >= kQuietCalls) {
    hipFree(*p);
    *p = nullptr;
    *cap = 0;
  }
}
static void trim_default_ctx(mib_ctx *c) {
  hipSetDevice(c->device);
  // (while a BrotliEncoder lives, its chunk after chunk reuses the workspace and the encoder
  // output stage: kept)
  const bool streaming = mib_live_encoders() > 0;
  for (int i = 0; i < kStageSlots; i++)
    if (!(streaming && i == 3)) release_large(&c->stage[i], &c->stage_cap[i], kKeepStage, c->stage_trim[i]);
  release_large(&c->d_scratch, &c->scratch_bytes, kKeepScratch, c->scratch_trim);
  release_large(&c->d_parts, &c->parts_bytes, kKeepScratch, c->parts_trim);
  release_large(&c->d_sspan, &c->sspan_bytes, kKeepStage, c->sspan_trim);
  if (!streaming) {
    mib_encode_ws_trim(&c->enc_ws, kKeepScratch);
    for (int l = 0; l < kEncLanes; l++) mib_encode_ws_trim(&c->lane_ws[l], kKeepScratch);
  }
}
// a context's buffers above these sizes (staging slots; decoder scratch, part tables and
// encoder workspace), released (multi.cpp's shard contexts after each sharded call)
void mib_ctx_trim(mib_ctx *c, uint64_t keep_stage, uint64_t keep_scratch) {
  hipSetDevice(c->device);
  for (int i = 0; i < kStageSlots; i++) release_large(&c->stage[i], &c->stage_cap[i], keep_stage, c->stage_trim[i]);
  release_large(&c->d_scratch, &c->scratch_bytes, keep_scratch, c->scratch_trim);
  release_large(&c->d_parts, &c->parts_bytes, keep_scratch, c->parts_trim);
  release_large(&c->d_sspan, &c->sspan_bytes, keep_stage, c->sspan_trim);
  mib_encode_ws_trim(&c->enc_ws, keep_scratch);
  for (int l = 0; l < kEncLanes; l++) mib_encode_ws_trim(&c->lane_ws[l], keep_scratch);
}
void mib_default_lock(int on) {
  if (on) {
    g_default_mu.lock();
    g_default_depth++;
  } else {
    if (--g_default_depth == 0 && g_default_ctx) trim_default_ctx(g_default_ctx);
    g_default_mu.unlock();
  }
}
namespace {
struct DefaultUse {   // mib_default_lock for this file's entry points
  DefaultUse() { mib_default_lock(1); }
  ~DefaultUse() { mib_default_lock(0); }
};
}  // namespace
int mib_ctx_ready(mib_ctx *c) { return c ? ensure_device(c->device) : MIB_E_INVALID_ARG; }
void *mib_ctx_stream_of(mib_ctx *c) { return (void *)c->stream; }
int mib_ctx_device_of(mib_ctx *c) { return c->device; }
void mib_ctx_clear_times(mib_ctx *c) { c->times.clear(); }

int mib_ctx_kernel_times(mib_ctx *c, mib_kernel_time *out, int max) {
  int n = std::min<int>(max, (int)c->times.size());
  for (int i = 0; i < n; i++) out[i] = c->times[i];
  return (int)c->times.size();
}

// A zeroed job: input, output and its capacity, the size known beforehand (or -1), the window
// bits that size the ring, and the stream's dictionary if it has one (dict_std: DecJob::dict_std)
static mib::DecJob dec_job(const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t out_cap, int64_t out_size, int lgwin,
                           const uint8_t *dict = nullptr, uint64_t dict_len = 0, int dict_std = 0) {
  mib::DecJob j;
  memset(&j, 0, sizeof(mib::DecJob));
  j.in = in, j.in_len = in_len, j.out = out, j.out_cap = out_cap, j.out_size = out_size, j.max_ring_log = lgwin;
  j.dict = dict, j.dict_len = dict_len, j.dict_std = dict_std;
  return j;
}

// One decode launch over jobs[] (not empty): scratch for `grid` blocks of per_block bytes, the
// jobs to the device, launch() -- which finds them in c->d_jobs and its scratch in c->d_scratch --
// timed under `name` when profiling, and the jobs back with what the kernel wrote into them.
static int launch_jobs(mib_ctx *c, std::vector<mib::DecJob> &jobs, uint64_t per_block, int grid, const char *name,
                       hipStream_t stream, const std::function<hipError_t()> &launch) {
  const size_t k = jobs.size();
  int rc;
  c->scratch_trim.need = std::max(c->scratch_trim.need, per_block * (uint64_t)grid);
  if ((rc = grow((void **)&c->d_scratch, &c->scratch_bytes, per_block * (uint64_t)grid)) != 0) return rc;
  if (k > c->jobs_cap) {
    if (c->d_jobs) hipFree(c->d_jobs);
    c->d_jobs = nullptr;
    c->jobs_cap = 0;
    if (hipMalloc(&c->d_jobs, sizeof(mib::DecJob) * k) != hipSuccess) return MIB_E_OUT_OF_MEMORY;
    c->jobs_cap = k;
  }
  HIP_OK(hipMemcpyAsync(c->d_jobs, jobs.data(), sizeof(mib::DecJob) * k, hipMemcpyHostToDevice, stream));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (c->profiling) {
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    hipEventRecord(e0, stream);
  }
  HIP_OK(launch());
  if (c->profiling) hipEventRecord(e1, stream);
  HIP_OK(hipMemcpyAsync(jobs.data(), c->d_jobs, sizeof(mib::DecJob) * k, hipMemcpyDeviceToHost, stream));
  HIP_OK(hipStreamSynchronize(stream));
  if (c->profiling) {
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    c->add_time(name, ms);
    hipEventDestroy(e0);
    hipEventDestroy(e1);
  }
  return 0;
}

// decode k streams whose bytes are on the device; jobs[] describes them (host copy)
static int decode_jobs(mib_ctx *c, std::vector<mib::DecJob> &jobs, hipStream_t stream) {
  size_t k = jobs.size();
  c->in_place_done = c->in_place_left = 0;
  if (k == 0) return 0;
  int max_log = 10;
  for (auto &j : jobs) max_log = std::max(max_log, j.max_ring_log);
  uint64_t ring_bytes = ((uint64_t)1 << max_log) + 37 + 256;
  ring_bytes = (ring_bytes + 255) & ~(uint64_t)255;
  uint64_t per_block = ring_bytes + mib::kDecodeScratchBytes;
  per_block = (per_block + 255) & ~(uint64_t)255;
  // (MIB_DEC_GRID: experiment knob, a smaller persistent grid -- fewer decoder waves per CU)
  static const size_t grid_cap = mib::knob("MIB_DEC_GRID") ? (size_t)std::max(1, atoi(mib::knob("MIB_DEC_GRID"))) : 2048;
  int grid = (int)std::min<size_t>(k, std::min<size_t>(grid_cap, 2048));
  const int rc = launch_jobs(c, jobs, per_block, grid, "decode_streams_kernel", stream, [&] {
    return mib_decode_launch(c->d_jobs, (int)k, c->d_scratch, per_block, ring_bytes, grid, waves_per_cu(c->device, (size_t)grid),
                             stream);
  });
  if (rc) return rc;
  for (auto &j : jobs) {
    c->in_place_done += j.in_place == 1 && j.status == 0;
    c->in_place_left += j.in_place == 2;
  }
  return 0;
}

// Decode indexed streams part-parallel.  streams[i] = (device input, length, device output,
// plan); ok[i] = 1 when every part of stream i checked out (its output is then complete:
// plan.total bytes), else the caller decodes it serially.
struct PartStream {
  const uint8_t *in;
  uint64_t in_len;
  uint8_t *out;
  const mib::PartPlan *plan;
  const uint8_t *dict;   // customDictionary (device), or null
  uint64_t dict_len;
  int dict_std;          // DecJob::dict_std
};
static int decode_parts(mib_ctx *c, const std::vector<PartStream> &ps, std::vector<int> &ok, hipStream_t stream) {
  size_t nj = 0, ne = 0;
  for (auto &p : ps) {
    nj += p.plan->ent.size();
    ne += p.plan->ent.size();
  }
  ok.assign(ps.size(), 0);
  if (nj == 0) return 0;
  // device layout: entries | positions (nparts + 1 per stream) | progress | ticket
  const uint64_t ent_b = ((ne * sizeof(mib::PartEntry)) + 255) & ~255ull;
  const uint64_t pos_b = (((ne + ps.size()) * 8) + 255) & ~255ull;
  const uint64_t prog_b = ((ne * 8) + 255) & ~255ull;
  int rc;
  c->parts_trim.need = std::max(c->parts_trim.need, ent_b + pos_b + prog_b + 256);
  if ((rc = grow((void **)&c->d_parts, &c->parts_bytes, ent_b + pos_b + prog_b + 256)) != 0) return rc;
  mib::PartEntry *d_ent = reinterpret_cast<mib::PartEntry *>(c->d_parts);
  int64_t *d_pos = reinterpret_cast<int64_t *>(c->d_parts + ent_b);
  uint64_t *d_prog = reinterpret_cast<uint64_t *>(c->d_parts + ent_b + pos_b);
  unsigned *d_ticket = reinterpret_cast<unsigned *>(c->d_parts + ent_b + pos_b + prog_b);
  std::vector<mib::PartEntry> ents;
  std::vector<int64_t> pos;
  std::vector<mib::DecJob> jobs;
  ents.reserve(ne);
  pos.reserve(ne + ps.size());
  jobs.reserve(nj);
  for (auto &p : ps) {
    const size_t e0 = ents.size(), p0 = pos.size();
    const size_t np = p.plan->ent.size();
    for (auto &x : p.plan->ent) {
      ents.push_back(x);
      pos.push_back((int64_t)x.pos);
    }
    pos.push_back(p.plan->total);
    for (size_t i = 0; i < np; i++) {
      mib::DecJob j = dec_job(p.in, p.in_len, p.out, (uint64_t)p.plan->total, p.plan->total, p.plan->lgwin, p.dict,
                              p.dict_len, p.dict_std);
      j.part_entry = d_ent + e0 + i;
      j.next_entry = i + 1 < np ? d_ent + e0 + i + 1 : nullptr;
      j.ppos = d_pos + p0;
      j.prog = d_prog + e0;
      j.pidx = (int32_t)i;
      j.nparts = (int32_t)np;
      j.total = p.plan->total;
      jobs.push_back(j);
    }
  }
  uint64_t per_block = mib::kDecodeScratchBytes;
  per_block = (per_block + 255) & ~(uint64_t)255;
  static const size_t grid_cap = mib::knob("MIB_PART_GRID") ? (size_t)std::max(1, atoi(mib::knob("MIB_PART_GRID"))) : 2048;
  const int grid = (int)std::min<size_t>(nj, grid_cap);
  HIP_OK(hipMemcpyAsync(d_ent, ents.data(), sizeof(mib::PartEntry) * ne, hipMemcpyHostToDevice, stream));
  HIP_OK(hipMemcpyAsync(d_pos, pos.data(), 8 * pos.size(), hipMemcpyHostToDevice, stream));
  HIP_OK(hipMemsetAsync(d_prog, 0, prog_b + 256, stream));   // progress words and the ticket
  rc = launch_jobs(c, jobs, per_block, grid, "decode_parts_kernel", stream, [&] {
    return mib_decode_parts_launch(c->d_jobs, (int)nj, c->d_scratch, per_block, d_ticket, grid,
                                   waves_per_cu(c->device, (size_t)grid), stream);
  });
  if (rc) return rc;
  size_t q = 0;
  for (size_t i = 0; i < ps.size(); i++) {
    int good = 1;
    for (size_t k = 0; k < ps[i].plan->ent.size(); k++, q++)
      if (jobs[q].status != 0) good = 0;
    ok[i] = good;
  }
  c->parts_used += ps.size();
  for (int v : ok) c->parts_fallback += v ? 0 : 1;
  return 0;
}

// mib_ctx_decode's body.  out_caps: stream i's capacity where its slot is longer than what it may
// write (slots padded to a boundary); null: the capacity is the slot, out_offsets[i + 1] -
// out_offsets[i].
static int decode_streams(mib_ctx *c, const uint8_t *d_in, const uint64_t *in_offsets, size_t k, uint8_t *d_out,
                          const uint64_t *out_offsets, const uint64_t *out_caps, int64_t *out_sizes, int *status,
                          void *stream) {
  if (!c || (k && (!d_in || !in_offsets || !d_out || !out_offsets))) return MIB_E_INVALID_ARG;
  if (ensure_device(c->device) != 0) return MIB_E_NO_DEVICE;
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  c->times.clear();
  std::vector<uint8_t> heads(16 * k + 16);
  std::vector<mib::DecJob> jobs(k);
  if (k) {   // window bits (and part index magic) of every stream, gathered in one launch
    int rc = grow((void **)&c->d_aux, &c->aux_bytes, (k + 1) * 8 + 16 * k + 256);
    if (rc) return rc;
    uint64_t *d_off = reinterpret_cast<uint64_t *>(c->d_aux);
    uint8_t *d_heads = c->d_aux + ((k + 1) * 8 + 255) / 256 * 256;
    HIP_OK(hipMemcpyAsync(d_off, in_offsets, (k + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_OK(mib_decode_peek_heads(d_in, d_off, (int)k, d_heads, st));
    HIP_OK(hipMemcpyAsync(heads.data(), d_heads, 16 * k, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
  }
  for (size_t i = 0; i < k; i++) {
    const uint64_t n = in_offsets[i + 1] - in_offsets[i];
    jobs[i] = dec_job(d_in + in_offsets[i], n, d_out + out_offsets[i], out_caps ? out_caps[i] : out_offsets[i + 1] - out_offsets[i],
                      -1, mib::peek_window_bits(&heads[16 * i], (size_t)std::min<uint64_t>(n, 2)));
  }
  // streams with a part index decode part-parallel; the rest (and any part stream that does
  // not check out) one wave per stream
  std::vector<mib::PartPlan> plans(k);
  std::vector<PartStream> ps;
  std::vector<size_t> ps_idx;
  std::vector<mib::DecJob> serial;
  std::vector<size_t> serial_idx;
  for (size_t i = 0; i < k; i++) {
    bool part = false;
    if (mib::looks_indexed(&heads[16 * i], jobs[i].in_len)) {
      DeviceFetch f{jobs[i].in, jobs[i].in_len, st};
      part = mib::plan_parts(f, jobs[i].in_len, plans[i]) && (uint64_t)plans[i].total + 64 <= jobs[i].out_cap;
    }
    if (part) {
      ps.push_back(PartStream{jobs[i].in, jobs[i].in_len, jobs[i].out, &plans[i], nullptr, 0, 0});
      ps_idx.push_back(i);
    } else {
      serial.push_back(jobs[i]);
      serial_idx.push_back(i);
    }
  }
  std::vector<int> ok;
  int rc = decode_parts(c, ps, ok, st);
  if (rc) return rc;
  for (size_t q = 0; q < ps.size(); q++) {
    const size_t i = ps_idx[q];
    if (ok[q]) {
      jobs[i].status = 0;
      jobs[i].result_len = plans[i].total;
    } else {
      serial.push_back(jobs[i]);
      serial_idx.push_back(i);
    }
  }
  rc = decode_jobs(c, serial, st);
  if (rc) return rc;
  for (size_t q = 0; q < serial.size(); q++) jobs[serial_idx[q]] = serial[q];
  int worst = 0;
  for (size_t i = 0; i < k; i++) {
    out_sizes[i] = jobs[i].result_len;
    status[i] = jobs[i].status;
    if (jobs[i].status) worst = jobs[i].status;
  }
  return worst == MIB_E_NEED_SPACE ? MIB_E_NEED_SPACE : 0;
}

int mib_ctx_decode(mib_ctx *c, const uint8_t *d_in, const uint64_t *in_offsets, size_t k, uint8_t *d_out,
                   const uint64_t *out_offsets, int64_t *out_sizes, int *status, void *stream) {
  return decode_streams(c, d_in, in_offsets, k, d_out, out_offsets, nullptr, out_sizes, status, stream);
}

// Internal (woff2_file.hip's batch): mib_ctx_decode with stream i's output at d_out +
// out_offsets[i] (k entries) and its capacity out_caps[i], whatever lies between the slots.
int mib_ctx_decode_caps(mib_ctx *c, const uint8_t *d_in, const uint64_t *in_offsets, size_t k, uint8_t *d_out,
                        const uint64_t *out_offsets, const uint64_t *out_caps, int64_t *out_sizes, int *status,
                        void *stream) {
  if (k && !out_caps) return MIB_E_INVALID_ARG;
  return decode_streams(c, d_in, in_offsets, k, d_out, out_offsets, out_caps, out_sizes, status, stream);
}

// one host stream through the device (brotliDecode semantics of decode.ts:18-65)
// (dict: host bytes, staged here; or, dict_dev, a dictionary resident on the device, with
// dict_std the rule its copies follow, DecJob::dict_std.  Caller: the default context held.)
static int decode_one(mib_ctx *c, const uint8_t *in, size_t n, const uint8_t *dict, size_t dict_n, const uint8_t *dict_dev,
                      int dict_std, int64_t max_out, int64_t exact_out, mib_buf *out) {
  int64_t out_size = -1;
  if (exact_out >= 0) {
    out_size = exact_out;   // legacy numeric signature: no peek (decode.ts:27-44)
  } else {
    int64_t est = mib_decoded_size(in, n);
    if (est > 0) out_size = est;
  }
  if (max_out >= 0 && out_size >= 0 && out_size > max_out) {
    out->size = (size_t)out_size;   // the size that exceeded the limit (decode.ts:46-50)
    return MIB_E_OUTPUT_LIMIT;
  }
  int known = out_size > 0;
  uint64_t cap = known ? (uint64_t)out_size : std::max<uint64_t>(1 << 20, 4 * (uint64_t)n + 4096);
  uint8_t *d_in = nullptr, *d_out = nullptr, *d_dict = nullptr;
  int rc = 0;
  if (!(d_in = mib_ctx_stage(c, 0, n + 16))) return MIB_E_OUT_OF_MEMORY;
  if (dict && !(d_dict = mib_ctx_stage(c, 2, dict_n + 16))) return MIB_E_OUT_OF_MEMORY;
  {
    const mib::HostPiece up[2] = {{d_in, in, n}, {d_dict, dict, dict ? dict_n : 0}};
    if ((rc = mib::ctx_upload(c, c->stream, up, dict ? 2 : 1))) return rc;
  }
  if (dict_dev) {
    d_dict = const_cast<uint8_t *>(dict_dev);   // (read only)
    dict = dict_dev;                            // (below: "has a dictionary")
  }
  if (exact_out < 0) {   // a stream with a part index: part-parallel, checked
    mib::PartPlan plan;
    mib::HostFetch f{in, n};
    // (the index is untrusted: a total beyond maxOutputSize, or one the device cannot hold,
    // just leaves the stream to the serial decoder, which finds out what it really is)
    if (mib::plan_parts(f, n, plan) && (max_out < 0 || plan.total <= max_out) &&
        (d_out = mib_ctx_stage(c, 1, (uint64_t)plan.total + 4096)) != nullptr) {
      std::vector<PartStream> ps(1);
      std::vector<int> ok;
      ps[0] = PartStream{d_in, n, d_out, &plan, d_dict, dict ? dict_n : 0, dict_std};
      rc = decode_parts(c, ps, ok, c->stream);
      if (rc == 0 && ok[0]) {
        return mib_buf_from_device(out, d_out, (uint64_t)plan.total);
      }
      rc = 0;
    }
  }
  for (;;) {
    // room for the ring of a one-metablock stream (a power of two >= its size, + slack), so
    // the kernel can decode in place instead of through its scratch ring (a stream with a
    // custom dictionary does so only when the whole ring fits: maybe_realloc_ring)
    uint64_t alloc = 1;
    while (alloc < cap) alloc <<= 1;
    alloc += 4096;
    if (!(d_out = mib_ctx_stage(c, 1, alloc))) {
      rc = MIB_E_OUT_OF_MEMORY;
      break;
    }
    std::vector<mib::DecJob> jobs(1);
    // (unknown size: cap is the growth step's limit)
    jobs[0] = dec_job(d_in, n, d_out, known ? alloc : cap, known ? out_size : -1, mib::peek_window_bits(in, n), d_dict,
                      dict ? dict_n : 0, dict_std);
    rc = decode_jobs(c, jobs, c->stream);
    if (rc) break;
    rc = jobs[0].status;
    if (rc == MIB_E_NEED_SPACE && !known && cap < ((uint64_t)1 << 31)) {   // JS caps a Uint8Array near 2^31
      cap *= 4;
      continue;
    }
    if (rc == 0) {
      uint64_t len = (uint64_t)jobs[0].result_len;
      if (max_out >= 0 && (int64_t)len > max_out) {   // the header can lie about the size (decode.ts:57-62)
        out->size = len;
        rc = MIB_E_OUTPUT_LIMIT;
      } else {
        rc = mib_buf_from_device(out, d_out, len);
      }
    }
    break;
  }
  return rc;
}

int mib_decode(const uint8_t *in, size_t n, const uint8_t *dict, size_t dict_n, int64_t max_out, int64_t exact_out,
               mib_buf *out) {
  if (!out || (!in && n)) return MIB_E_INVALID_ARG;
  out->data = nullptr;
  out->size = 0;
  DefaultUse use;
  mib_ctx *c = default_ctx();
  if (!c) return MIB_E_NO_DEVICE;
  hipSetDevice(c->device);
  return decode_one(c, in, n, dict, dict_n, nullptr, 0, max_out, exact_out, out);
}

// The body of mib_decode_batch (d null, max_out -1) and mib_decode_batch_dictionary: the streams in
// one launch, each in a slot sized by what its header announces (or guessed: decode_plan.h
// plan_batch), with the dictionary and the standard rule if there is one; the streams that outgrew
// their slots, and those the alone rules single out, one by one through decode_one.
static int decode_batch(const mib_span *in, size_t k, const mib_dictionary *d, int64_t max_out, mib_buf *out, int *status) {
  static const bool timing = mib::knob("MIB_HOST_TIMING") != nullptr;
  const auto t_in = std::chrono::steady_clock::now();
  auto ms_since = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_in).count(); };
  DefaultUse use;
  mib_ctx *c = default_ctx();
  if (!c) return MIB_E_NO_DEVICE;
  if (d && d->device != c->device) return MIB_E_INVALID_ARG;
  hipSetDevice(c->device);
  // The two calls differ in routing, and only here.  With a dictionary handle a part-indexed stream
  // goes alone, and so decodes part-parallel (decode_one), as does a stream whose header announces
  // more than kBatchSlotMax; without one both stay in the launch, the indexed stream on one wave, the
  // announced size uncapped.  (Whether the plain call should adopt either rule has not been measured.)
  const bool alone_rules = d != nullptr;
  const mib::BatchLayout lay = mib::plan_batch(in, k, max_out, alone_rules);
  std::vector<uint8_t> alone(k, 0);
  std::vector<mib::HostPiece> up;
  std::vector<mib::DecJob> jobs;
  std::vector<size_t> slot;
  for (size_t i = 0; i < k; i++) {
    const mib::BatchItem &t = lay.item[i];
    alone[i] = t.how == mib::kAlone;
    if (t.how == mib::kInLaunch) slot.push_back(i);
    if (t.how == mib::kSettled) status[i] = MIB_E_OUTPUT_LIMIT, out[i].size = (size_t)t.est;
  }
  uint8_t *d_in = nullptr, *d_out = nullptr;
  if (!slot.empty()) {
    d_in = mib_ctx_stage(c, 0, lay.in_bytes + 16), d_out = mib_ctx_stage(c, 1, lay.out_bytes + 64);
    if (!d_in || !d_out) return MIB_E_OUT_OF_MEMORY;
  }
  up.reserve(slot.size()), jobs.reserve(slot.size());
  for (size_t i : slot) {   // exact input lengths, padded slots
    const mib::BatchItem &t = lay.item[i];
    if (in[i].size) up.push_back(mib::HostPiece{d_in + t.in_off, in[i].data, in[i].size});
    jobs.push_back(dec_job(d_in + t.in_off, in[i].size, d_out + t.out_off, t.out_slot - 64, t.est > 0 ? t.est : -1,
                           mib::peek_window_bits(in[i].data, in[i].size), d ? d->d_data : nullptr, d ? d->n : 0, d ? 1 : 0));
  }
  int rc = 0;
  if (!up.empty() && (rc = mib::ctx_upload(c, c->stream, up.data(), up.size()))) return rc;
  const double t_up = timing ? ms_since() : 0.0;
  if (!jobs.empty()) rc = decode_jobs(c, jobs, c->stream);
  const double t_dec = timing ? ms_since() : 0.0;
  std::vector<mib_buf *> outs;
  std::vector<const uint8_t *> src;
  std::vector<uint64_t> lens;
  for (size_t q = 0; q < jobs.size() && rc == 0; q++) {
    const size_t i = slot[q];
    status[i] = jobs[q].status;
    if (jobs[q].status == MIB_E_NEED_SPACE) {
      alone[i] = 1;
    } else if (jobs[q].status == 0) {
      const uint64_t len = (uint64_t)jobs[q].result_len;
      if (max_out >= 0 && (int64_t)len > max_out) {   // (the header can lie about the size)
        status[i] = MIB_E_OUTPUT_LIMIT;
        out[i].size = len;
      } else {
        outs.push_back(&out[i]);
        src.push_back(d_out + lay.item[i].out_off);
        lens.push_back(len);
      }
    }
  }
  if (!outs.empty() && (rc = mib_bufs_from_device(outs.size(), outs.data(), src.data(), lens.data())))
    for (size_t i = 0; i < k; i++) mib_buf_free(&out[i]);
  // (the staging buffers are reused from here on: the growing single-stream path)
  for (size_t i = 0; i < k && rc == 0; i++)
    if (alone[i]) {
      status[i] = decode_one(c, in[i].data, in[i].size, nullptr, d ? d->n : 0, d ? d->d_data : nullptr, d ? 1 : 0, max_out, -1,
                             &out[i]);
      if (status[i] != 0 && status[i] != MIB_E_OUTPUT_LIMIT) out[i].data = nullptr, out[i].size = 0;
    }
  if (timing)
    fprintf(stderr, "[mib] decode_batch %zu streams: upload done %.2f ms, decode done %.2f, results %.2f\n", k, t_up, t_dec,
            ms_since());
  return rc;
}

// what both batch calls ask of their arguments; clears out[] and status[]
static int batch_args(const mib_span *in, size_t k, mib_buf *out, int *status) {
  if (k && (!in || !out || !status)) return MIB_E_INVALID_ARG;
  for (size_t i = 0; i < k; i++) {
    out[i].data = nullptr, out[i].size = 0, status[i] = 0;
    if (!in[i].data && in[i].size) return MIB_E_INVALID_ARG;
  }
  return 0;
}

int mib_decode_batch_dictionary(const mib_span *in, size_t k, const mib_dictionary *d, int64_t max_out, mib_buf *out,
                                int *status) {
  if (!d || max_out < -1 || batch_args(in, k, out, status)) return MIB_E_INVALID_ARG;
  return k ? decode_batch(in, k, d, max_out, out, status) : 0;
}

int mib_decode_batch(const mib_span *in, size_t k, mib_buf *out, int *status) {
  if (batch_args(in, k, out, status)) return MIB_E_INVALID_ARG;
  return k ? decode_batch(in, k, nullptr, -1, out, status) : 0;
}

}  // extern "C"

// ---------------------------------------------------------------- streaming decoder
// A session keeps in HBM its dictionary, the session buffer (history, a window of new output,
// slack: stream_session.h) and the pending input (from the oldest byte a resume reads again),
// and between launches the checkpoint.  update() appends its bytes to the pending input and
// launches decode_resume_kernel until a launch suspends for input; a launch that stops on the
// output limit has its bytes copied out and the history moved to the buffer's front first
// (mib::stream_rounds, which decides everything over the StreamSession part below).  What a
// launch needs besides -- decode scratch, its job, the checkpoint's head -- is the context's.
struct mib_decoder : mib::StreamSession {
  std::vector<uint8_t> dict;          // customDictionary until the device copy exists
  bool has_dict = false;
  // or a prepared dictionary (mib_decoder_new_dictionary): has_dict, d_dict is the handle's own
  // device memory (never freed here), no host copy; the session holds a reference (dictionary.h)
  const mib_dictionary *handle = nullptr;
  uint64_t dict_len() const { return handle ? handle->n : has_dict ? dict.size() : 0; }
  uint8_t *d_dict = nullptr, *d_buf = nullptr, *d_in = nullptr;
  uint64_t in_cap = 0;
  mib::StreamCkpt *d_ck = nullptr;    // the window dump lives here; every launch carries the head beside its job
  int device = 0;
};

namespace {
int g_force_small_decoder = 0;   // mib_force_decoder_build
constexpr size_t kCkHead = mib::kStreamCkHead;
static_assert(kCkHead == offsetof(mib::StreamCkpt, win), "the checkpoint head ends where the window starts");
constexpr uint64_t kStreamScratch = (mib::kDecodeScratchBytes + 255) & ~(uint64_t)255;

void decoder_release(mib_decoder *d) {
  hipSetDevice(d->device);
  for (void *p : {(void *)(d->handle ? nullptr : d->d_dict), (void *)d->d_buf, (void *)d->d_in, (void *)d->d_ck})
    if (p) hipFree(p);
  d->d_dict = d->d_buf = d->d_in = nullptr;
  d->d_ck = nullptr;
  d->buf_cap = d->in_cap = d->in_len = 0;
  d->deliv = d->held_to = 0;
  d->due = false;
}

// the stream's first byte is here: its window sizes the session buffer
int decoder_open(mib_decoder *d, mib_ctx *c, uint8_t first) {
  const int lgwin = mib::stream_window_bits(first);
  if (lgwin < 0) return -11;   // the reserved window-bits pattern (engine.ts decodeWindowBits)
  d->lgwin = lgwin;
  d->buf_cap = mib::stream_buf_cap(lgwin, d->out_window);
  if (hipMalloc((void **)&d->d_buf, d->buf_cap) != hipSuccess || hipMalloc((void **)&d->d_ck, sizeof(mib::StreamCkpt)) != hipSuccess)
    return MIB_E_OUT_OF_MEMORY;
  if (d->handle) {   // resident: the handle's bytes, in place
    if (d->handle->device != c->device) return MIB_E_INVALID_ARG;
    d->d_dict = d->handle->d_data;
  } else if (d->has_dict) {
    if (hipMalloc((void **)&d->d_dict, d->dict.size() + 16) != hipSuccess) return MIB_E_OUT_OF_MEMORY;
    const mib::HostPiece up{d->d_dict, d->dict.data(), d->dict.size()};
    int rc = mib::ctx_upload(c, c->stream, &up, 1);
    if (rc) return rc;
  }
  mib::stream_initial_ckpt(&d->ck, lgwin);
  HIP_OK(hipMemcpyAsync(d->d_ck, &d->ck, sizeof(d->ck), hipMemcpyHostToDevice, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));   // (d->ck / d->dict are read by the copies)
  return 0;
}

// room for n more bytes of pending input
int decoder_reserve(mib_decoder *d, mib_ctx *c, size_t n) {
  if (d->in_len + n + 16 > d->in_cap) {
    const uint64_t cap = std::max<uint64_t>(2 * d->in_cap, std::max<uint64_t>(d->in_len + n + 16, 1 << 16));
    uint8_t *p = nullptr;
    if (hipMalloc((void **)&p, cap) != hipSuccess) return MIB_E_OUT_OF_MEMORY;
    if (d->in_len) {
      if (hipMemcpyAsync(p, d->d_in, d->in_len, hipMemcpyDeviceToDevice, c->stream) != hipSuccess ||
          hipStreamSynchronize(c->stream) != hipSuccess) {
        hipFree(p);
        return MIB_E_NO_DEVICE;
      }
    }
    if (d->d_in) hipFree(d->d_in);
    d->d_in = p;
    d->in_cap = cap;
  }
  return 0;
}

int decoder_result(mib_decoder *d, int rc, std::vector<uint8_t> &got, mib_buf *out) {
  if (rc == 0) {
    out->data = mib_buf_alloc(got.size());
    if (!out->data) rc = MIB_E_OUT_OF_MEMORY;
    else {
      out->size = got.size();
      if (!got.empty()) memcpy(out->data, got.data(), got.size());
    }
  }
  if (rc) {
    d->error = rc;   // every later call reports it; the device memory goes now
    if (rc == MIB_E_OUTPUT_LIMIT) out->size = (size_t)d->total_out;
    decoder_release(d);
  }
  return rc;
}

// ---------------------------------------------------------------- the rounds of a call
// This file's part of mib::stream_rounds (RoundsDev below).  However many sessions, a round is one
// upload (jobs, checkpoint heads, move descriptors), one move launch, one decode launch, one
// read-back, and for what the sessions then deliver ONE copy launch -- into the callers' device
// ranges, or into the staging span, which comes down in one copy.
uint64_t g_batch_launches = 0;   // mib_decoder_batch_stats
int g_decoder_grid_cap = 0;      // mib_force_decoder_grid
double g_batch_ms[5];            // mib_decoder_batch_times: upload, launch, read-back, delivery launch, download

// descriptors to the front of the context's batch buffer (whose content goes) and the copy
// launches over them (stream_batch.h plan_copies); asynchronous on the context's stream
int copy_batch(mib_ctx *c, const std::vector<mib::CopyDesc> &cd) {
  if (cd.empty()) return 0;
  int rc;
  if ((rc = grow((void **)&c->d_sbatch, &c->sbatch_bytes, cd.size() * sizeof(mib::CopyDesc))) != 0) return rc;
  HIP_OK(hipMemcpyAsync(c->d_sbatch, cd.data(), cd.size() * sizeof(mib::CopyDesc), hipMemcpyHostToDevice, c->stream));
  std::vector<mib::CopyLaunch> ls;
  mib::plan_copies(cd.data(), cd.size(), mib::kGatherMaxDescs, ls);
  for (const mib::CopyLaunch &l : ls)
    HIP_OK(mib_stream_copy_batch_launch((const mib::CopyDesc *)c->d_sbatch + l.first, (uint32_t)l.count, l.blocks, c->stream));
  return 0;
}

double ms_between(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
  return std::chrono::duration<double, std::milli>(b - a).count();
}

// Where a call's chunks come from and where its bytes go: host memory (in, out) or, for the
// device-resident calls, ranges of two device buffers given by host offset arrays.
struct BatchIo {
  const mib_span *in = nullptr;
  mib_buf *out = nullptr;
  bool device = false;
  const uint8_t *d_in = nullptr;
  const uint64_t *in_offsets = nullptr;
  uint8_t *d_out = nullptr;
  const uint64_t *out_offsets = nullptr;
  uint64_t *out_sizes = nullptr;
  size_t chunk(size_t i, bool finish) const {
    return finish ? 0 : device ? (size_t)(in_offsets[i + 1] - in_offsets[i]) : in[i].size;
  }
};

// The device's part of a call's rounds (mib::stream_rounds decides, this does): slot i is
// session d[i].  It also takes the timestamps of the five legs (mib_decoder_batch_times).
struct RoundsDev {
  using clk = std::chrono::steady_clock;
  mib_ctx *c;
  mib_decoder *const *d;
  const BatchIo &io;
  std::vector<uint8_t> host, span;
  std::vector<mib::MoveDesc> moves;
  std::vector<mib::MoveUnit> units;
  std::vector<mib::CopyDesc> cd;
  std::vector<uint64_t> dst;
  clk::time_point t3 = clk::now();   // where the delivery leg starts: the end of the read-back, or of the last round

  // the moves' descriptors at host[at] and their blocks (plan_moves) behind them; `host` goes up
  // to the front of the context's batch buffer and the moves run
  int run_moves(uint64_t at) {
    mib::plan_moves(moves.data(), moves.size(), units);
    const uint64_t units_at = (at + moves.size() * sizeof(mib::MoveDesc) + 15) & ~15ull;
    host.resize(units_at + units.size() * sizeof(mib::MoveUnit));
    if (!moves.empty()) memcpy(host.data() + at, moves.data(), moves.size() * sizeof(mib::MoveDesc));
    if (!units.empty()) memcpy(host.data() + units_at, units.data(), units.size() * sizeof(mib::MoveUnit));
    int rc;
    if ((rc = grow((void **)&c->d_sbatch, &c->sbatch_bytes, host.size())) != 0) return rc;
    HIP_OK(hipMemcpyAsync(c->d_sbatch, host.data(), host.size(), hipMemcpyHostToDevice, c->stream));
    return mib_stream_move_batch_launch((const mib::MoveDesc *)(c->d_sbatch + at), (const mib::MoveUnit *)(c->d_sbatch + units_at),
                                        (uint32_t)units.size(), c->stream) == hipSuccess ? 0 : MIB_E_NO_DEVICE;
  }

  // One round's decode launch over the slots `jobs`, each of which holds nothing: the histories
  // move, the jobs go up, ONE launch runs them, jobs and checkpoint heads come back.
  int launch(const std::vector<size_t> &jobs, const std::vector<mib::StreamPlan> &plans, int final, mib::StreamJob *ret,
             uint8_t *heads) {
    const auto t0 = clk::now();
    const int cus = (c->device >= 0 && c->device < kMaxDevices && g_dev_cus[c->device] > 0) ? g_dev_cus[c->device] : 256;
    int rc;
    const size_t k = jobs.size();
    // [jobs][heads][move descriptors][move units]: one upload; the first two come back
    const uint64_t heads_at = mib::stream_heads_offset(k, sizeof(mib::StreamJob));
    const uint64_t moves_at = (heads_at + k * kCkHead + 15) & ~15ull;
    host.assign(moves_at, 0);
    moves.clear();
    for (size_t a = 0; a < k; a++) {
      const mib_decoder *s = d[jobs[a]];
      // the history to the buffer's front: the launch needs out_window + slack behind pos
      if (plans[a].move) moves.push_back(mib::MoveDesc{s->d_buf, plans[a].move, s->ck.e.pos});
      // (in, in_len, buf, buf_cap, out_limit, dict, dict_len, ck, lgwin, final, status, dict_std; the kernel's fields 0)
      const mib::StreamJob j{s->d_in, s->in_len, s->d_buf, s->buf_cap, plans[a].out_limit, s->d_dict,
                             s->dict_len(), s->d_ck, s->lgwin, final, 0, s->handle ? 1 : 0, 0, 0, 0};
      memcpy(host.data() + a * sizeof(j), &j, sizeof(j));
      memcpy(host.data() + heads_at + a * kCkHead, &s->ck, kCkHead);
    }
    const int per_cu = __atomic_load_n(&g_force_small_decoder, __ATOMIC_RELAXED) ? 4 : waves_per_cu(c->device, k);
    const int grid = mib::stream_batch_grid(k, cus, per_cu, __atomic_load_n(&g_decoder_grid_cap, __ATOMIC_RELAXED));
    c->scratch_trim.need = std::max(c->scratch_trim.need, kStreamScratch * (uint64_t)grid);
    if ((rc = grow((void **)&c->d_scratch, &c->scratch_bytes, kStreamScratch * (uint64_t)grid)) != 0) return rc;
    if ((rc = run_moves(moves_at)) != 0) return rc;
    const auto t1 = clk::now();
    HIP_OK(mib_decode_resume_launch((mib::StreamJob *)c->d_sbatch, (int)k, c->d_scratch, kStreamScratch, grid, per_cu,
                                    c->d_sbatch + heads_at, c->stream));
    __atomic_add_fetch(&g_batch_launches, 1, __ATOMIC_RELAXED);
    // (waiting here, not in the copy, costs nothing -- the copy into pageable memory waits for the
    // launch anyway -- and lets mib_decoder_batch_times tell the launch from the read-back)
    HIP_OK(hipStreamSynchronize(c->stream));
    const auto t2 = clk::now();
    HIP_OK(hipMemcpyAsync(host.data(), c->d_sbatch, heads_at + k * kCkHead, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    memcpy(ret, host.data(), k * sizeof(mib::StreamJob));
    memcpy(heads, host.data() + heads_at, k * kCkHead);
    t3 = clk::now();
    g_batch_ms[0] += ms_between(t0, t1);
    g_batch_ms[1] += ms_between(t1, t2);
    g_batch_ms[2] += ms_between(t2, t3);
    return 0;
  }

  // One copy launch for every slot's bytes: into the callers' ranges (nothing comes down), or
  // into the staging span (plan_gather), which comes down in one copy and is cut into `got`.
  int deliver(std::vector<mib::StreamSlot> &slots, const std::vector<size_t> &who, const std::vector<uint64_t> &len) {
    if (who.empty()) return 0;
    int rc;
    uint64_t total = 0;
    if (!io.device) {
      dst.resize(who.size());
      total = mib::plan_gather(len.data(), len.size(), dst.data());
      c->sspan_trim.need = std::max(c->sspan_trim.need, total);
      if ((rc = grow((void **)&c->d_sspan, &c->sspan_bytes, total)) != 0) return rc;
    }
    cd.clear();
    for (size_t g = 0; g < who.size(); g++) {
      const size_t i = who[g];
      cd.push_back(mib::CopyDesc{d[i]->d_buf + d[i]->deliv,
                                 io.device ? io.d_out + io.out_offsets[i] + slots[i].given : c->d_sspan + dst[g], len[g]});
    }
    if ((rc = copy_batch(c, cd)) != 0) return rc;   // (the descriptors take the place of the jobs, which are read)
    if (io.device) HIP_OK(hipStreamSynchronize(c->stream));   // (a host call waits in its download)
    const auto t4 = clk::now();
    if (!io.device) {
      span.resize(total);
      const mib::HostPiece down{span.data(), c->d_sspan, total};
      if ((rc = mib::ctx_download(c, c->stream, &down, 1)) != 0) return rc;
      for (size_t g = 0; g < who.size(); g++) {
        std::vector<uint8_t> &got = slots[who[g]].got;
        got.insert(got.end(), span.begin() + dst[g], span.begin() + dst[g] + len[g]);
      }
      g_batch_ms[4] += ms_between(t4, clk::now());
    }
    g_batch_ms[3] += ms_between(t3, t4);
    t3 = clk::now();
    return 0;
  }

  // every session's input move in one launch: in[0, in_len) <- in[drop, drop + in_len)
  int move_inputs(const std::vector<size_t> &who, const std::vector<uint64_t> &drop) {
    int rc;
    moves.clear();
    for (size_t g = 0; g < who.size(); g++) moves.push_back(mib::MoveDesc{d[who[g]]->d_in, drop[g], d[who[g]]->in_len});
    host.clear();
    if ((rc = run_moves(0)) != 0) return rc;
    HIP_OK(hipStreamSynchronize(c->stream));
    return 0;
  }
};

// The first byte of each of the chunks `open` (slots whose session has not seen a byte yet): its
// window bits size the session buffer on the host.  One copy launch collects them behind its
// descriptors, one read-back brings them.
int fetch_first_bytes(mib_ctx *c, const BatchIo &io, const std::vector<size_t> &open, std::vector<uint8_t> &first) {
  first.assign(open.size(), 0);
  if (open.empty()) return 0;
  const uint64_t at = (open.size() * sizeof(mib::CopyDesc) + 15) & ~15ull;
  int rc;
  if ((rc = grow((void **)&c->d_sbatch, &c->sbatch_bytes, at + open.size())) != 0) return rc;
  std::vector<mib::CopyDesc> cd;
  for (size_t j = 0; j < open.size(); j++) cd.push_back(mib::CopyDesc{io.d_in + io.in_offsets[open[j]], c->d_sbatch + at + j, 1});
  if ((rc = copy_batch(c, cd)) != 0) return rc;
  HIP_OK(hipMemcpyAsync(first.data(), c->d_sbatch + at, open.size(), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  return 0;
}

// update or finish of k sessions, already checked (decoder_batch_check)
int decoder_batch(mib_decoder *const *d, const BatchIo &io, size_t k, int *status, bool finish) {
  // what each session does in this call; a call whose sessions all return without a launch or a
  // delivery (failed, finished, nothing to add, nothing held) needs no device
  std::vector<mib::StreamAdmit> admit(k);
  std::vector<size_t> open;   // the slots whose session opens on a chunk in device memory
  bool device = false;
  for (size_t i = 0; i < k; i++) {
    admit[i] = mib::stream_admit(*d[i], io.chunk(i, finish), finish);
    if (mib::stream_admit_needs_device(admit[i], *d[i])) device = true;
    if (io.device && !finish && admit[i] == mib::StreamAdmit::kFeed && !d[i]->lgwin) open.push_back(i);
  }
  std::unique_ptr<DefaultUse> hold;   // (the default context for the whole call, taken only when a session needs the device)
  mib_ctx *c = nullptr;
  if (device) {
    hold.reset(new DefaultUse);
    c = default_ctx();
    if (!c) return MIB_E_NO_DEVICE;
    hipSetDevice(c->device);
  }
  std::vector<mib::StreamSlot> slots(k);
  std::vector<mib::HostPiece> up;
  std::vector<mib::CopyDesc> app;
  std::vector<uint8_t> first;
  int rc = fetch_first_bytes(c, io, open, first);
  size_t opened = 0;
  for (size_t i = 0; i < k; i++) {
    mib::StreamSlot &s = slots[i];
    s.s = d[i];
    status[i] = 0;
    if (io.device) {
      io.out_sizes[i] = 0;
      s.room = io.out_offsets[i + 1] - io.out_offsets[i];
    } else io.out[i] = mib_buf{nullptr, 0};
    mib::stream_admit_slot(s, admit[i]);
    if (admit[i] != mib::StreamAdmit::kNothing && !d[i]->finished) d[i]->device = c->device;
    if (admit[i] != mib::StreamAdmit::kFeed) continue;
    const size_t n = io.chunk(i, finish);
    if (rc) { s.rc = rc; continue; }   // the first bytes did not come: the call fails below
    // no byte at all (finish): the decoder reads an empty input's padding, window bits 0 (16) first
    if (!d[i]->lgwin) s.rc = decoder_open(d[i], c, finish ? 0 : io.device ? first[opened++] : io.in[i].data[0]);
    if (!s.rc) s.rc = decoder_reserve(d[i], c, n);
    if (s.rc) continue;
    if (n) {
      if (io.device) app.push_back(mib::CopyDesc{io.d_in + io.in_offsets[i], d[i]->d_in + d[i]->in_len, n});
      else up.push_back(mib::HostPiece{d[i]->d_in + d[i]->in_len, io.in[i].data, n});
    }
    d[i]->in_len += n;
    s.run = true;
  }
  // every slot's chunk behind its session's pending input: one copy launch, or the host's pieces
  if (!rc && !app.empty()) rc = copy_batch(c, app);
  if (!rc && !up.empty()) rc = mib::ctx_upload(c, c->stream, up.data(), up.size());
  if (!rc && c) {
    RoundsDev dev{c, d, io};
    rc = mib::stream_rounds(dev, slots, finish ? 1 : 0);
  }
  for (size_t i = 0; i < k; i++) {
    mib::StreamSlot &s = slots[i];
    if (d[i]->error) { status[i] = d[i]->error; continue; }
    if (rc && (s.run || mib::held(*d[i]))) s.rc = rc;   // a device failure ends the sessions that still had work
    if (!io.device) {
      status[i] = decoder_result(d[i], s.rc, s.got, &io.out[i]);
    } else if (s.rc) {
      mib_buf none{nullptr, 0};
      status[i] = decoder_result(d[i], s.rc, s.got, &none);
      io.out_sizes[i] = none.size;   // (MIB_E_OUTPUT_LIMIT: the total, as in the host call)
    } else {
      io.out_sizes[i] = s.given;
      status[i] = mib::stream_more_output(mib::held(*d[i]), s.room, d[i]->due) ? MIB_DEC_MORE_OUTPUT : 0;
    }
  }
  return 0;
}

// what every batch call checks before it touches a session
int decoder_batch_check(mib_decoder *const *d, size_t k) {
  if (!d) return MIB_E_INVALID_ARG;
  for (size_t i = 0; i < k; i++)
    if (!d[i]) return MIB_E_INVALID_ARG;
  std::vector<const mib_decoder *> seen(d, d + k);
  std::sort(seen.begin(), seen.end());
  return std::adjacent_find(seen.begin(), seen.end()) != seen.end() ? MIB_E_INVALID_ARG : 0;
}

int decoder_batch_host(mib_decoder *const *d, const mib_span *in, size_t k, mib_buf *out, int *status, bool finish) {
  if (k == 0) return 0;
  if (!out || !status || (!finish && !in) || decoder_batch_check(d, k)) return MIB_E_INVALID_ARG;
  for (size_t i = 0; i < k; i++)
    if (!finish && !in[i].data && in[i].size) return MIB_E_INVALID_ARG;
  return decoder_batch(d, BatchIo{in, out}, k, status, finish);
}

int decoder_batch_device(mib_decoder *const *d, const uint8_t *d_in, const uint64_t *in_offsets, size_t k, uint8_t *d_out,
                         const uint64_t *out_offsets, uint64_t *out_sizes, int *status, bool finish) {
  if (k == 0) return 0;
  if (!out_offsets || !out_sizes || !status || (!finish && !in_offsets) || decoder_batch_check(d, k)) return MIB_E_INVALID_ARG;
  for (size_t i = 0; i < k; i++)
    if (out_offsets[i + 1] < out_offsets[i] || (!finish && in_offsets[i + 1] < in_offsets[i])) return MIB_E_INVALID_ARG;
  if ((!d_out && out_offsets[k] > out_offsets[0]) || (!finish && !d_in && in_offsets[k] > in_offsets[0])) return MIB_E_INVALID_ARG;
  return decoder_batch(d, BatchIo{nullptr, nullptr, true, d_in, in_offsets, d_out, out_offsets, out_sizes}, k, status, finish);
}
}  // namespace

extern "C" {

int mib_decoder_update_batch(mib_decoder *const *d, const mib_span *in, size_t k, mib_buf *out, int *status) {
  if (k && !in) return MIB_E_INVALID_ARG;
  return decoder_batch_host(d, in, k, out, status, false);
}

int mib_decoder_finish_batch(mib_decoder *const *d, size_t k, mib_buf *out, int *status) {
  return decoder_batch_host(d, nullptr, k, out, status, true);
}

int mib_decoder_update_batch_device(mib_decoder *const *d, const uint8_t *d_in, const uint64_t *in_offsets, size_t k,
                                    uint8_t *d_out, const uint64_t *out_offsets, uint64_t *out_sizes, int *status) {
  return decoder_batch_device(d, d_in, in_offsets, k, d_out, out_offsets, out_sizes, status, false);
}

int mib_decoder_finish_batch_device(mib_decoder *const *d, size_t k, uint8_t *d_out, const uint64_t *out_offsets,
                                    uint64_t *out_sizes, int *status) {
  return decoder_batch_device(d, nullptr, nullptr, k, d_out, out_offsets, out_sizes, status, true);
}

uint64_t mib_decoder_held_output(const mib_decoder *d) { return d && !d->error ? d->held_to - d->deliv : 0; }

// Diagnostic: the copy kernel alone, over host arrays of device pointers
int mib_debug_copy_batch(const uint8_t *const *d_src, uint8_t *const *d_dst, const uint64_t *n, size_t k) {
  if (k == 0) return 0;
  if (!d_src || !d_dst || !n) return MIB_E_INVALID_ARG;
  std::vector<mib::CopyDesc> cd;
  for (size_t i = 0; i < k; i++) {
    if (n[i] && (!d_src[i] || !d_dst[i])) return MIB_E_INVALID_ARG;
    cd.push_back(mib::CopyDesc{d_src[i], d_dst[i], n[i]});
  }
  DefaultUse use;
  mib_ctx *c = default_ctx();
  if (!c) return MIB_E_NO_DEVICE;
  hipSetDevice(c->device);
  const int rc = copy_batch(c, cd);
  if (rc) return rc;
  HIP_OK(hipStreamSynchronize(c->stream));
  return 0;
}

void mib_decoder_batch_stats(uint64_t *launches) {
  if (launches) *launches = __atomic_load_n(&g_batch_launches, __ATOMIC_RELAXED);
}

void mib_decoder_batch_times(double *ms, int n) {
  for (int i = 0; ms && i < n; i++) ms[i] = i < 5 ? g_batch_ms[i] : 0;
}

void mib_force_decoder_grid(int max_blocks) { __atomic_store_n(&g_decoder_grid_cap, max_blocks > 0 ? max_blocks : 0, __ATOMIC_RELAXED); }

void mib_dec_opts_default(mib_dec_opts *o) {
  if (!o) return;
  o->dict = nullptr;
  o->dict_len = 0;
  o->max_out = -1;
  o->out_window = 0;
}

mib_decoder *mib_decoder_new(const mib_dec_opts *o) {
  mib_dec_opts def;
  mib_dec_opts_default(&def);
  if (!o) o = &def;
  if ((!o->dict && o->dict_len) || o->max_out < -1) return nullptr;
  mib_decoder *d = new mib_decoder();
  d->max_out = o->max_out;
  d->out_window = mib::stream_clamp_window(o->out_window);
  if (o->dict) {   // (an empty dictionary is still attached, as in brotliDecode)
    d->has_dict = true;
    d->dict.assign(o->dict, o->dict + o->dict_len);
  }
  return d;
}

mib_decoder *mib_decoder_new_dictionary(const mib_dec_opts *o, const mib_dictionary *h) {
  if (!h || (o && o->dict)) return nullptr;   // (before any device work, and before h is read)
  mib_decoder *d = mib_decoder_new(o);
  if (!d) return nullptr;
  mib_dictionary_ref(h);
  d->handle = h;
  d->has_dict = true;
  return d;
}

// a lone session's calls are the batch calls with k = 1 (`out` is emptied here: a call that
// finds no device returns before it touches its slots)
int mib_decoder_update(mib_decoder *d, const uint8_t *in, size_t n, mib_buf *out) {
  if (!d || !out || (!in && n)) return MIB_E_INVALID_ARG;
  out->data = nullptr;
  out->size = 0;
  const mib_span s{in, n};
  int status = 0;
  const int rc = decoder_batch_host(&d, &s, 1, out, &status, false);
  return rc ? rc : status;
}

int mib_decoder_finish(mib_decoder *d, mib_buf *out) {
  if (!d || !out) return MIB_E_INVALID_ARG;
  out->data = nullptr;
  out->size = 0;
  int status = 0;
  const int rc = decoder_batch_host(&d, nullptr, 1, out, &status, true);
  return rc ? rc : status;
}

int mib_decoder_is_finished(const mib_decoder *d) { return d && d->finished && !d->error; }

void mib_decoder_stats(const mib_decoder *d, uint64_t *passes, uint64_t *redecoded) {
  if (passes) *passes = d ? d->passes : 0;
  if (redecoded) *redecoded = d ? d->redone : 0;
}

void mib_force_decoder_build(int four_per_cu) { __atomic_store_n(&g_force_small_decoder, four_per_cu ? 1 : 0, __ATOMIC_RELAXED); }

void mib_decoder_free(mib_decoder *d) {
  if (!d) return;
  if (d->d_buf || d->d_in || d->d_dict) {
    DefaultUse use;
    decoder_release(d);
  }
  if (d->handle) mib_dictionary_unref(d->handle);
  delete d;
}

}  // extern "C"

extern "C" void mib_force_ballot_rank(int force) { __atomic_store_n(&g_force_ballot, force ? 1 : 0, __ATOMIC_RELAXED); }
// internal (multi.cpp): give back the context's pinned transfer ring (allocated again on the
// next large transfer)
extern "C" void mib_ctx_release_ring(mib_ctx *c) {
  if (!c || !c->ring) return;
  hipSetDevice(c->device);
  hipStreamSynchronize(c->stream);
  hipHostFree(c->ring);
  c->ring = nullptr;
  for (int h = 0; h < 2; h++)
    if (c->ring_ev[h]) {
      hipEventDestroy(c->ring_ev[h]);
      c->ring_ev[h] = nullptr;
    }
}
