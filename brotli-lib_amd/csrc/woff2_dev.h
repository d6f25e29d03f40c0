// What the WOFF2 host entry points (woff2.hip, woff2_inv.hip, woff2_file.hip, woff2_write.hip)
// share: a call's device buffers, its per-kernel timer, the scope every entry point runs in on
// the default context (Call), and the transform and reconstruct cores that work on device memory.
#ifndef MIB_WOFF2_DEV_H_
#define MIB_WOFF2_DEV_H_
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <utility>
#include <vector>

#include "common.h"

extern "C" mib_ctx *mib_default_ctx(void);
extern "C" void mib_default_lock(int on);
extern "C" void *mib_ctx_stream_of(mib_ctx *c);
extern "C" int mib_ctx_device_of(mib_ctx *c);
extern "C" int mib_ctx_profiling(mib_ctx *c);
extern "C" void mib_ctx_add_time(mib_ctx *c, const char *name, double ms);

namespace mib {
namespace woff2dev {

struct Timer {   // per-kernel device time when the context profiles (mib_ctx_set_profiling)
  mib_ctx *c;
  hipStream_t s;
  bool on;
  std::vector<std::pair<const char *, std::pair<hipEvent_t, hipEvent_t>>> ev;
  void start(const char *name) {
    if (!on) return;
    hipEvent_t a, b;
    hipEventCreate(&a);
    hipEventCreate(&b);
    hipEventRecord(a, s);
    ev.push_back({name, {a, b}});
  }
  void stop() {
    if (on) hipEventRecord(ev.back().second.second, s);
  }
  void collect(bool ok) {
    for (auto &e : ev) {
      float ms = 0;
      if (ok && hipEventElapsedTime(&ms, e.second.first, e.second.second) == hipSuccess)
        mib_ctx_add_time(c, e.first, ms);
      hipEventDestroy(e.second.first);
      hipEventDestroy(e.second.second);
    }
    ev.clear();
  }
};

// The call's device buffers, freed together.  Each has 16 bytes of slack behind it: what a
// 16-byte vector read of its last bytes may touch (load16.h).
struct DevMem {
  std::vector<void *> p;
  template <class T>
  T *take(size_t count) {
    void *q = nullptr;
    if (hipMalloc(&q, sizeof(T) * (count ? count : 1) + 16) != hipSuccess) return nullptr;
    p.push_back(q);
    return (T *)q;
  }
  ~DevMem() {
    for (void *q : p) hipFree(q);
  }
};

inline void drop(mib_buf *b) {   // a result the call does not return after all
  if (b->data) mib_buf_free(b);
  b->data = nullptr;
  b->size = 0;
}

// One call of an entry point on the default context: the context's lock, its device set, its
// stream, a timer and the call's buffers.  An entry point that holds one leaves with
// `return use.rc = <code>`: on a non-zero rc the destructor synchronises the stream, so that
// nothing of the call is in flight when its buffers go, and the timer's entries count only where
// the entry point said `timed`.  After the destructor the members die in reverse order: the
// buffers, and last the lock.
struct Call {
  struct Lock {   // (recursive: the decode and encode calls on this context run inside it)
    Lock() { mib_default_lock(1); }
    ~Lock() { mib_default_lock(0); }
  } lock;
  mib_ctx *c;   // null: no device
  hipStream_t st;
  Timer tm;     // on where the entry point times its kernels and the context profiles
  DevMem m;
  int rc = 0;
  bool timed = false;
  explicit Call(bool timing)
      : c(mib_default_ctx()), st(c ? (hipStream_t)mib_ctx_stream_of(c) : nullptr),
        tm{c, st, timing && c && mib_ctx_profiling(c) == 1, {}} {
    if (c) hipSetDevice(mib_ctx_device_of(c));
  }
  Call(const Call &) = delete;
  ~Call() {
    if (rc && c) hipStreamSynchronize(st);
    tm.collect(timed);
  }
  // n bytes of device memory into a fresh mib_buf, synchronised; *out is empty on failure
  int fetch(const uint8_t *d, size_t n, mib_buf *out) {
    out->size = 0;
    if (!(out->data = mib_buf_alloc(n))) return MIB_E_OUT_OF_MEMORY;
    out->size = n;
    hipMemcpyAsync(out->data, d, n, hipMemcpyDeviceToHost, st);
    if (hipStreamSynchronize(st) == hipSuccess) return 0;
    drop(out);
    return MIB_E_NO_DEVICE;
  }
};

// The glyf reconstruct's work between upload and download.  The caller holds the default
// context's lock, has set its device, and owns the DevMems and `tm`.
// Return codes as the entry point's; on 0 the stream has been synchronised.
//   the transformed table's n bytes at d_t, `hdr` a host copy of its first 36 (woff2_inv.h
//   parse_header has to have accepted hdr, n).  loca follows glyf in memory.  The results live
//   in `keep`, everything else in `m`: once the stream has been synchronised after the call, `m`
//   may go before the results are used (the two may be one DevMem).
int reconstruct_glyf_device(hipStream_t st, Timer &tm, DevMem &m, DevMem &keep, const uint8_t *hdr, const uint8_t *d_t,
                            size_t n, uint8_t **d_glyf, size_t *glyf_b, uint8_t **d_loca, size_t *loca_b);

// One font of the hmtx launch (blockIdx.y), all on the device: the transformed table's n >= 1
// bytes at t (its flags and size are checked on the device), the font's glyf and loca, and out of
// 4 * nhm + 2 * (ng - nhm) bytes.  The caller has checked ng, nhm and loca's size (hmtx_shape_ok).
struct HmtxFont {
  const uint8_t *t;
  uint64_t n;
  const uint8_t *glyf, *loca;
  uint8_t *out;
  uint32_t glyf_n, long_loca, ng, nhm;
};
// One launch ("w2inv_hmtx") over k >= 1 fonts whose descriptors are at d_fonts; most_ng: the
// largest ng among them.  d_bad[f] (zeroed by the caller) is raised for a font whose flags do not
// fit its size or whose loca does not fit its glyf.  Nothing is synchronised.
void launch_hmtx(hipStream_t st, Timer &tm, const HmtxFont *d_fonts, size_t k, uint32_t most_ng, int *d_bad);

// The transform cores (woff2.hip): what mib_woff2_transform_glyf / _hmtx do between upload and
// download, and what the file writer (woff2_write.hip) runs per font.  Each has a sizing step,
// which synchronises the stream and tells how many bytes the table takes, and a write step, which
// writes them -- the 36-byte header and the hmtx flag byte included -- at a device address of any
// alignment and synchronises nothing.  The caller holds the default context's lock and has set its
// device; what the sizing step took from `m` has to live until the write step's kernels are done.
struct GlyfIn {   // glyf and loca on the device, any alignment; loca holds num_glyphs + 1 entries
  const uint8_t *d_glyf;
  uint32_t glyf_len;
  const uint8_t *d_loca;
  uint32_t num_glyphs, long_loca;
};
struct GlyfSized {
  GlyfIn in;
  const uint32_t *d_offs;   // the scanned per-glyph stream sizes
  const uint8_t *d_bits;    // per glyph: overlap-simple, explicit bbox
  uint32_t base[7], bbox_at;
  uint64_t streams_end;
  bool overlap;
  uint64_t total;           // the transformed table's bytes
  uint8_t header[36];
};
//   MIB_E_INVALID_ARG: a malformed glyph
int transform_glyf_size(hipStream_t st, Timer &tm, DevMem &m, const GlyfIn &in, GlyfSized *z);
void transform_glyf_write(hipStream_t st, Timer &tm, const GlyfSized &z, uint8_t *d_out);
struct HmtxSized {
  const uint8_t *d_hmtx;
  uint32_t num_glyphs, nhm, keep;
  uint64_t total;   // 0: both side-bearing arrays differ from the glyphs' xMin -- no transform
};
//   d_hmtx: at least 4 nhm + 2 (num_glyphs - nhm) bytes, 1 <= nhm <= num_glyphs
int transform_hmtx_size(hipStream_t st, Timer &tm, DevMem &m, const GlyfIn &in, const uint8_t *d_hmtx, uint32_t nhm,
                        HmtxSized *z);
void transform_hmtx_write(hipStream_t st, Timer &tm, const HmtxSized &z, uint8_t *d_out);

}  // namespace woff2dev

namespace woff2file {
uint64_t forced_group_bytes();   // mib_force_woff2_group_bytes' value (woff2_file.hip)
}
}  // namespace mib
#endif
