// The rounds of the streaming decoder's calls (DESIGN.md §4d "Rounds"): every decision of a
// call -- what a slot does in it, who launches, who delivers and how much, who goes on, what a
// launch that came back means for its session, when pending input is compacted -- over the
// part of a session they read and write.  Plain C++ (no HIP types): the device work is a template
// parameter, runtime.cpp's launches and copies in the product and a model session in
// tests/stream_deliver_host_main.cpp, so the loop the sanitizers run is the product's.
// What a launch decoded is first HELD by its session, buf[deliv, held_to), and then delivered: a
// host call's slot has no limit and takes everything, a device-resident call's slot min(held,
// room left).  A session that holds bytes only delivers in a round and gets a job only with
// nothing held and room left, so the history moves with nothing held.  A slot whose range is full
// leaves holding the rest, or owing its launch (`due`), for the next call of either kind.
#pragma once
#include "../../include/brotli_amd.h"
#include "stream_batch.h"
#include "stream_session.h"

namespace mib {

struct StreamSession {
  int64_t max_out = -1;
  uint64_t out_window = 0, buf_cap = 0, in_len = 0;
  StreamCkpt ck;                      // host mirror (its window stays on the device)
  int lgwin = 0;                      // 0: the stream's first byte has not arrived
  uint64_t total_out = 0, passes = 0, redone = 0;   // redone: output bytes decoded twice (behind a checkpoint)
  uint64_t need_len = 0;              // pending bytes the next launch needs at least (0: unknown)
  uint64_t deliv = 0, held_to = 0;
  bool due = false;                   // input or finish() that has seen no launch yet, or the last launch left on kStreamNeedOutput
  int error = 0;
  bool finished = false;
};
inline uint64_t held(const StreamSession &s) { return s.held_to - s.deliv; }

struct StreamSlot {
  StreamSession *s = nullptr;
  int rc = 0;
  bool run = false;       // has a launch to make in the next round (after the last: an input move to wait for)
  bool suspended = false; // left on kStreamNeedInput: its pending input may be compacted
  std::vector<uint8_t> got;   // a host call's slot: its bytes
  uint64_t room = kNoRoomLimit, given = 0;   // what the slot's range still takes / has been given
};

// ---------------------------------------------------------------- admission
enum class StreamAdmit {
  kNothing,    // failed, or nothing to add and nothing pending: returns 0 and no bytes
  kDeliver,    // only hands out what it holds
  kTrailing,   // a chunk for a finished session: -17, as one-shot decoding refuses bytes behind the end
  kFeed,       // opens if no byte has come yet, appends its chunk, launches
  kDue,        // launches for input or a finish() an earlier call had no room for
};
// what a session does in a call that brings it n bytes (finish: none, and no more come)
inline StreamAdmit stream_admit(const StreamSession &s, uint64_t n, bool finish) {
  if (s.error) return StreamAdmit::kNothing;
  const bool pending = held(s) || s.due;
  if (!pending && (finish ? s.finished : n == 0)) return StreamAdmit::kNothing;
  if (s.finished) return n ? StreamAdmit::kTrailing : StreamAdmit::kDeliver;
  if (finish || n) return StreamAdmit::kFeed;
  return s.due ? StreamAdmit::kDue : StreamAdmit::kDeliver;
}
// ... and whether that takes the device (a refused chunk: only to let go of held bytes)
inline bool stream_admit_needs_device(StreamAdmit a, const StreamSession &s) {
  return a == StreamAdmit::kTrailing ? held(s) > 0 : a != StreamAdmit::kNothing;
}
// the slot's part of it (kFeed: the caller appends the chunk, adds it to in_len and sets `run`)
inline void stream_admit_slot(StreamSlot &slot, StreamAdmit a) {
  if (a == StreamAdmit::kTrailing) slot.rc = -17;
  if (a == StreamAdmit::kDue) slot.run = true;
}

// What a session's launch is given: the history buf[move, move + pos) goes to the buffer's front
// first (move = 0: it stays), then the launch leaves at the first boundary at or behind out_limit.
// The session holds nothing: its positions are rebased and its held range is empty at pos.
struct StreamPlan {
  uint64_t out_limit, move;
};
inline StreamPlan stream_plan_launch(StreamSession &s, StreamSlot &slot) {
  const uint64_t delta = stream_compact_delta(s.ck.e.pos, s.lgwin);
  if (delta) stream_rebase_output(&s.ck, delta);
  s.deliv = s.held_to = s.ck.e.pos;
  return StreamPlan{stream_out_limit(s.deliv, s.out_window, slot.room), delta};
}

// A launch came back with job j and checkpoint head `head`: its pass counts, an error ends the
// session, its new bytes are [deliv, out_pos) and count against max_out (a session over its limit
// returns none of them), and its status says whether the session is done, failed, has a further
// launch to make (`run`) or waits for input (`suspended`).
inline void stream_account(StreamSession &s, StreamSlot &slot, const StreamJob &j, const uint8_t *head, bool final) {
  memcpy(&s.ck, head, kStreamCkHead);
  s.passes++;
  slot.run = false;
  if (j.status == kStreamNeedInput && j.redone > 0) s.redone += (uint64_t)j.redone;
  if (j.status < 0) { slot.rc = j.status; return; }
  if (j.out_pos < (int64_t)s.deliv || (uint64_t)j.out_pos > s.buf_cap) { slot.rc = MIB_E_NO_PROGRESS; return; }
  s.total_out += (uint64_t)j.out_pos - s.deliv;
  if (s.max_out >= 0 && s.total_out > (uint64_t)s.max_out) { slot.rc = MIB_E_OUTPUT_LIMIT; return; }
  s.held_to = (uint64_t)j.out_pos;
  if (j.status == kStreamNeedInput && !final) s.need_len = j.need_len > 0 ? (uint64_t)j.need_len : 0;
  if (j.status == kStreamFinished) {
    s.finished = true;
    // bytes behind the stream's end: refused, as one-shot decoding refuses them (-17)
    if (s.in_len > ((s.ck.e.bit + 7) >> 3)) slot.rc = -17;
  } else if (j.status == kStreamNeedOutput) {   // (the checkpoint is where the launch left)
    slot.run = true;
  } else if (j.status != kStreamNeedInput || final) {
    slot.rc = MIB_E_NO_PROGRESS;
  } else {
    slot.suspended = true;
  }
}

// Input no resume reads again leaves the front of a suspended session's pending bytes once it is
// worth a move: at least 64 KiB, and at least half of what is pending.  Returns how many bytes
// leave (0: none) and rebases the session; moving in[drop, drop + in_len) down is the caller's.
constexpr uint64_t kStreamInputDropMin = 64u << 10;
inline uint64_t stream_compact_input(StreamSession &s) {
  const uint64_t keep = stream_keep_from(s.ck);
  if (keep < kStreamInputDropMin || 2 * keep < s.in_len) return 0;
  s.in_len -= keep;
  s.need_len = s.need_len > keep ? s.need_len - keep : 0;
  stream_rebase_input(&s.ck, keep);   // (the session's next launch brings the rebased head)
  return keep;
}

// ---------------------------------------------------------------- the rounds
// The rounds of one call over its admitted slots.  Dev does the device's part, decides nothing:
//   int launch(jobs, plans, final, StreamJob *ret, uint8_t *heads)   the slots jobs[a], moved and
//       limited as plans[a] says, in ONE launch; ret[a] is the job as the kernel left it,
//       heads + a * kStreamCkHead the checkpoint head it wrote
//   int deliver(slots, who, len)   len[g] bytes from `deliv` of slot who[g]'s session to its caller
//   int move_inputs(who, drop)     drop[g] bytes leave the front of slot who[g]'s pending input
// A non-zero return is a device failure; it ends every session still in a round.
template <class Dev>
int stream_rounds(Dev &dev, std::vector<StreamSlot> &slots, int final) {
  std::vector<size_t> act, jobs, who, next;
  for (size_t i = 0; i < slots.size(); i++) {
    StreamSlot &s = slots[i];
    if (s.rc) continue;
    // the last launch stopped in front of a raw or metadata block that is still not whole
    if (s.run && !stream_enters_round(final != 0, s.s->in_len, s.s->need_len)) s.run = false;
    if ((s.run || held(*s.s)) && s.room > 0) act.push_back(i);
  }
  std::vector<StreamPlan> plans;
  std::vector<StreamJob> ret;
  std::vector<uint8_t> heads;
  std::vector<uint64_t> len;
  int rc;
  while (!act.empty()) {
    // who launches: the sessions that hold nothing, have room left and a launch to make
    jobs.clear();
    plans.clear();
    for (size_t i : act)
      if (stream_plans_job(held(*slots[i].s), slots[i].room, slots[i].run)) {
        jobs.push_back(i);
        plans.push_back(stream_plan_launch(*slots[i].s, slots[i]));
      }
    if (!jobs.empty()) {
      ret.resize(jobs.size());
      heads.resize(jobs.size() * kStreamCkHead);
      if ((rc = dev.launch(jobs, plans, final, ret.data(), heads.data())) != 0) return rc;
      for (size_t a = 0; a < jobs.size(); a++)
        stream_account(*slots[jobs[a]].s, slots[jobs[a]], ret[a], heads.data() + a * kStreamCkHead, final != 0);
    }
    // who delivers: every session of the round that holds bytes, min(held, room left) of them
    who.clear();
    len.clear();
    for (size_t i : act) {
      const uint64_t n = slots[i].rc ? 0 : deliver_len(held(*slots[i].s), slots[i].room);
      if (n) {
        who.push_back(i);
        len.push_back(n);
      }
    }
    if ((rc = dev.deliver(slots, who, len)) != 0) return rc;
    for (size_t g = 0; g < who.size(); g++) {
      StreamSlot &s = slots[who[g]];
      s.s->deliv += len[g];
      s.room -= len[g];   // (kNoRoomLimit stays out of reach: a session buffer is below 2^30)
      s.given += len[g];
    }
    // who goes on: a launch to make or bytes held, and room for them
    next.clear();
    for (size_t i : act)
      if (!slots[i].rc && (slots[i].run || held(*slots[i].s)) && slots[i].room > 0) next.push_back(i);
    act.swap(next);
  }
  // a slot whose range ran out before its launch could be made owes it to the next call
  for (StreamSlot &s : slots)
    if (!s.s->error) s.s->due = s.run && !s.rc;
  // every suspended session's input move in one launch
  who.clear();
  len.clear();
  for (size_t i = 0; i < slots.size(); i++) {
    StreamSlot &s = slots[i];
    const uint64_t drop = s.suspended && !s.rc ? stream_compact_input(*s.s) : 0;
    if (drop) {
      who.push_back(i);
      len.push_back(drop);
      s.run = true;   // until the move is done: a device failure in it ends this session too
    }
  }
  if (!who.empty()) {
    if ((rc = dev.move_inputs(who, len)) != 0) return rc;
    for (StreamSlot &s : slots) s.run = false;
  }
  return 0;
}

}  // namespace mib
