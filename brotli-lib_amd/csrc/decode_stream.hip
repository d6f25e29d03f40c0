// brotli_amd: the streaming sessions' decode kernel (decode_resume_kernel), a
// translation unit of its own over the decoder's device functions (decode_core.inc).
//
// Why not one more kernel in decode.hip's unit: the decoder's device functions are shared by
// every kernel of their unit, and a further kernel changes how the compiler builds them for all --
// hot_loop<false> loses the propagated constant of its one call site (stop_at_boundary = 0;
// +12 VGPRs in all four product kernels), and the file-scope LDS variables are laid out anew
// for the unit's kernels (every shared function grew, fast_loop included, +1 VGPR in the four
// kernels).  Compiled here, the sessions' kernel gets its own copies and decode.hip's kernels
// are, instruction for instruction, what they were.
#define MIB_TU_VAR static
#include "decode_core.inc"
#include "load16.h"
#include "stream_batch.h"

namespace mib {

// ---------------------------------------------------------------- streaming sessions
// One launch of a session (stream_session.h): enter at the checkpoint as a
// part does, put the bit reader back exactly, decode command by command until the input or
// the output limit says stop, and write the last covered boundary back as the checkpoint.
//
// The session buffer is the ring, as a part's output is: ring_size = 2^30 is above every
// position in it (stream_session.h's static_assert), so no `& rmask` wraps and no fence is
// reached, and ring_cap is the buffer's real capacity.  Stores: literals are clamped by
// ring_cap (hot_loop); a copy is refused (-9) when longer than the metablock's rest, which
// the slack behind out_limit holds; dictionary words, compound copies and uncompressed
// metablocks are checked in decompress<true>.  Positions: part_start = 0, so literal contexts
// read the buffer (the history is in it) and no copy source counts as another part's.
__device__ int stream_run(DecS &s, const StreamJob &job, StreamCtl *c, int8_t *dist_extra, int32_t *dist_offset,
                          int32_t *ctxmap_table) {
  StreamCkpt *ck = job.ck;
  const PartEntry e = ck->e;
  const int64_t win_off = ck->win_off;
  const int ho = ck->ho, bo = ck->bo;
  const uint32_t acc0 = ck->acc;
  if (job.lgwin < 10 || job.lgwin > 24 || job.buf_cap >= (1ull << 30) || win_off < 0 || (uint64_t)win_off > job.in_len ||
      ho < 0 || ho > 2080 || bo < 0 || bo > 32)
    return MIB_E_INVALID_ARG;
  s.part = 1;
  s.max_ring = 1 << job.lgwin;
  s.max_back = s.max_ring - 16;
  s.ring = job.buf;
  s.direct = kDirectRing;
  s.ring_size = 1 << 30;
  s.ring_cap = (int)job.buf_cap;
  s.expected_total = 1 << 30;
  s.known_size = 1;
  if (entry_load(s, e, dist_extra, dist_offset, ctxmap_table) < 0) return MIB_E_NO_PROGRESS;
  if ((e.flags & kPartAtMb) && (e.flags & kStreamInputEnd)) s.input_end = 1;
  // The reader, exactly: the window as it was last filled (stale bytes and all), the bytes the
  // input has by now over it, and (ho, bo); acc holds the half-words ho - 2 and ho - 1, taken
  // from the window again where they lie in it (they may have been padding when saved).
  wave_sync();
  const uint64_t have = job.in_len - (uint64_t)win_off;
  const int n = have < (uint64_t)kStreamWin ? (int)have : kStreamWin;
  for (int k = LANE; k < kStreamWin; k += 64) g_lds.win[k] = k < n ? job.in[win_off + k] : ck->win[k];
  for (int k = kStreamWin + LANE; k < (int)sizeof(g_lds.win); k += 64) g_lds.win[k] = 0;
  wave_sync();
  s.in_off = (uint64_t)win_off + (uint64_t)n;
  s.eos = n < kStreamWin;
  s.tail = s.eos ? n : 0;
  s.win_base = win_off;
  s.ho = ho;
  s.bo = bo;
  const uint32_t h0 = ho >= 2 ? half_at(s, ho - 2) : (acc0 & 0xFFFFu);
  const uint32_t h1 = ho >= 1 ? half_at(s, ho - 1) : (acc0 >> 16);
  s.acc = (h1 << 16) | h0;
  if (LANE == 0) {
    c->in_bits = 8 * (int64_t)job.in_len;
    c->out_limit = (int)job.out_limit;
    c->final = job.final;
    c->ck = ck;
    c->dumped_off = win_off;
    c->cur_mb_bit = (int64_t)e.mb_bit;
    c->bit = -1;   // no boundary yet
    c->need_len = 0;
    c->pos = (int)(int64_t)e.pos;
  }
  wave_sync();
  int r = decompress<true>(s, dist_extra, dist_offset, ctxmap_table, c);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  wave_sync();
  int status;
  if (r == 1) status = kStreamFinished;
  else if (r == 3 + kStreamNeedInput || r == 3 + kStreamNeedOutput) status = r - 3;
  // an error met after the reader ran out of this launch's input may be the missing bytes'
  else if (r < 0) status = (!job.final && s.eos) ? kStreamNeedInput : r;
  else status = MIB_E_NO_PROGRESS;
  if (LANE == 0 && c->bit >= 0) {
    PartEntry o;
    o.bit = (uint64_t)c->bit;
    o.pos = (uint64_t)(int64_t)c->pos;
    o.mb_bit = (uint64_t)c->mb_bit;
    o.mb_pos = (uint64_t)(int64_t)c->mb_pos;
    for (int k = 0; k < 4; k++) o.ring[k] = (uint32_t)c->ring[k];
    for (int k = 0; k < 3; k++) {
      o.blen[k] = (uint32_t)c->blen[k];
      o.type[k] = (uint8_t)c->type[k];
      o.prev[k] = (uint8_t)c->prev[k];
    }
    o.p1 = c->pos >= 1 ? job.buf[c->pos - 1] : 0;
    o.p2 = c->pos >= 2 ? job.buf[c->pos - 2] : 0;
    o.flags = (uint32_t)c->flags;
    ck->e = o;
    ck->win_off = c->win_off;
    ck->ho = c->ho;
    ck->bo = c->bo;
    ck->acc = c->acc;
  }
  return status;
}

template <bool BIG>
__global__ __launch_bounds__(64) void decode_resume_kernel(StreamJob *jobs, int njobs, uint8_t *scratch, uint64_t per_block,
                                                               uint8_t *heads) {
  constexpr int tab_cap = BIG ? kLdsTabBig : kLdsTab;
  __shared__ uint16_t tab[tab_cap];
  __shared__ int32_t bt_lds[BIG ? kBlockTreesCap + 1 : 1];
  __shared__ StreamCtl ctl;
  uint8_t *base = scratch + (uint64_t)blockIdx.x * per_block;
  int32_t *tables = reinterpret_cast<int32_t *>(base);
  uint8_t *ctx = reinterpret_cast<uint8_t *>(tables + kDecodeTableInts);
  int8_t *dist_extra = reinterpret_cast<int8_t *>(ctx + kDecodeCtxBytes);
  int32_t *dist_offset = reinterpret_cast<int32_t *>(dist_extra + 1152);
  int32_t *ctxmap_table = dist_offset + 1152;
  int32_t *block_trees = BIG ? bt_lds : ctxmap_table + 1100;
  for (int jb = blockIdx.x; jb < njobs; jb += gridDim.x) {
    const StreamJob job = jobs[jb];
    // A launch carries the checkpoint heads beside its jobs, so the host sends and fetches them
    // in one copy each: the head goes to the session's checkpoint here and comes back below.
    // The block's waves share one CU, so the barrier orders the stores.
    uint64_t *slot = reinterpret_cast<uint64_t *>(heads + (uint64_t)jb * kStreamCkHead);
    if (LANE < (int)(kStreamCkHead / 8)) reinterpret_cast<uint64_t *>(job.ck)[LANE] = slot[LANE];
    __syncthreads();
    DecJob dj;
    dj.in = job.in;
    dj.in_len = job.in_len;
    dj.out = job.buf;
    dj.out_cap = job.buf_cap;   // (with in_len: the launch's iteration guard, dec_init)
    dj.out_size = -1;
    dj.dict = job.dict;
    dj.dict_len = job.dict_len;
    dj.dict_std = job.dict_std;   // (a session made with a handle: the standard rule; else the reference's)
    DecS &s = *(DecS *)&g_dec;
    dec_init(s, dj, job.buf, tables, ctx, block_trees, tab, tab_cap);
    const int status = stream_run(s, job, &ctl, dist_extra, dist_offset, ctxmap_table);
    if (LANE == 0) {
      jobs[jb].status = status;
      // finished: everything decoded; suspended: up to the checkpoint (what a command that
      // ran out of input wrote behind it is decoded again)
      jobs[jb].need_len = status == kStreamNeedInput ? ctl.need_len : 0;
      jobs[jb].redone = status == kStreamNeedInput && s.pos > ctl.pos ? (int64_t)s.pos - ctl.pos : 0;
      jobs[jb].out_pos = status == kStreamFinished ? (int64_t)s.pos : status > 0 ? (int64_t)ctl.pos : 0;
    }
    __syncthreads();
    if (LANE < (int)(kStreamCkHead / 8)) slot[LANE] = reinterpret_cast<const uint64_t *>(job.ck)[LANE];
  }
}

// ---------------------------------------------------------------- moves and copies (stream_batch.h)
// One tile of a copy dst[0, n) <- src[0, n), laid over dst's 16-byte granules (stream_batch.h
// tiles_of): this thread's granule is loaded, the block meets, the granule is stored.  A
// granule that lies whole in [0, n) moves as one vector, the head and tail granules byte-wise.
template <int THREADS>
__device__ __forceinline__ void copy_tile(uint8_t *dst, const uint8_t *src, uint64_t n, uint64_t tile) {
  const uint64_t mis = (uint64_t)((uintptr_t)dst & 15);
  const uint64_t g = tile * THREADS + threadIdx.x;
  const int64_t lo = (int64_t)(16 * g) - (int64_t)mis;   // the granule's first byte, as an offset in [0, n)
  const bool whole = lo >= 0 && (uint64_t)lo + 16 <= n;
  uint4 v = make_uint4(0, 0, 0, 0);
  uint8_t b[16];
  if (whole) {
    v = load16_any(src + lo);
  } else {
#pragma unroll
    for (int q = 0; q < 16; q++) b[q] = lo + q >= 0 && (uint64_t)(lo + q) < n ? src[lo + q] : 0;
  }
  __syncthreads();
  if (whole) {
    *reinterpret_cast<uint4 *>(dst + lo) = v;
  } else {
#pragma unroll
    for (int q = 0; q < 16; q++)
      if (lo + q >= 0 && (uint64_t)(lo + q) < n) dst[lo + q] = b[q];
  }
  __syncthreads();
}

// Every due move of a round in one launch.  Block b does units[b]: the tiles tile0, tile0 +
// step, ... of one descriptor in ascending order, each loaded whole before it is stored, so a
// tile's stores (below its own sources, src > 0) cannot reach what a LATER tile of the same
// block still has to read.  The host gives an overlapping move (src < n) one block, which then
// owns every tile; without overlap no store lands in the source range and any split is safe
// (stream_batch.h plan_moves).
__global__ __launch_bounds__(kMoveThreads) void stream_move_batch_kernel(const MoveDesc *descs, const MoveUnit *units) {
  const MoveUnit u = units[blockIdx.x];
  const MoveDesc d = descs[u.desc];
  const uint64_t tiles = tiles_of((uint64_t)(uintptr_t)d.buf, d.n, kMoveTile);
  for (uint64_t t = u.tile0; t < tiles; t += u.step) copy_tile<kMoveThreads>(d.buf, d.buf + d.src, d.n, t);
}

// dst[0, n) <- src[0, n) for every descriptor (blockIdx.y), its tiles over blockIdx.x.  Source
// and destination have any alignment and are pointers of their own, so the tiles are counted
// over the destination's granules from its misalignment.  Two destinations may share a
// 16-byte granule: a granule that is not whole inside [0, n) is written byte by byte, by its
// own descriptor only (copy_tile), so neither touches the other's bytes or anything outside.
__global__ __launch_bounds__(kGatherThreads) void stream_copy_batch_kernel(const CopyDesc *descs) {
  const CopyDesc d = descs[blockIdx.y];
  const uint64_t tiles = tiles_of((uint64_t)(uintptr_t)d.dst, d.n, kGatherTile);
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) copy_tile<kGatherThreads>(d.dst, d.src, d.n, t);
}

}  // namespace mib

// d_heads: njobs checkpoint heads of kStreamCkHead bytes, which the kernel reads and writes
extern "C" hipError_t mib_decode_resume_launch(mib::StreamJob *d_jobs, int njobs, uint8_t *d_scratch, uint64_t per_block,
                                               int grid, int per_cu, uint8_t *d_heads, hipStream_t stream) {
  if (!d_heads) return hipErrorInvalidValue;
  if (per_cu <= 1)
    hipLaunchKernelGGL(mib::decode_resume_kernel<true>, dim3(grid), dim3(64), 0, stream, d_jobs, njobs, d_scratch, per_block, d_heads);
  else
    hipLaunchKernelGGL(mib::decode_resume_kernel<false>, dim3(grid), dim3(64), 0, stream, d_jobs, njobs, d_scratch, per_block, d_heads);
  return hipGetLastError();
}

// n_units blocks (stream_batch.h plan_moves); both arrays on the device
extern "C" hipError_t mib_stream_move_batch_launch(const mib::MoveDesc *d_descs, const mib::MoveUnit *d_units, uint32_t n_units,
                                                   hipStream_t stream) {
  if (n_units == 0) return hipSuccess;
  hipLaunchKernelGGL(mib::stream_move_batch_kernel, dim3(n_units), dim3(mib::kMoveThreads), 0, stream, d_descs, d_units);
  return hipGetLastError();
}

// k descriptors (<= kGatherMaxDescs), `blocks` blocks each (stream_batch.h plan_copies)
extern "C" hipError_t mib_stream_copy_batch_launch(const mib::CopyDesc *d_descs, uint32_t k, uint32_t blocks, hipStream_t stream) {
  if (k == 0) return hipSuccess;
  hipLaunchKernelGGL(mib::stream_copy_batch_kernel, dim3(blocks, k), dim3(mib::kGatherThreads), 0, stream, d_descs);
  return hipGetLastError();
}

// this translation unit's copy of the command table (mib_decode_init_tables, per device)
extern "C" hipError_t mib_decode_stream_init_tables(const int16_t *host_lut) {
  return hipMemcpyToSymbol(HIP_SYMBOL(mib::kCmdLut), host_lut, sizeof(int16_t) * 704 * 4);
}

