// The rounds of the session calls (brotli-lib_amd/csrc/stream_rounds.h: admission, who launches
// and with which output limit, the accounting of a launch, how much a slot delivers and what
// stays held, input compaction; stream_batch.h: the copy launches' grids and their split) driven
// with seeded random sessions and rooms, stand-alone so that it runs under AddressSanitizer and
// UBSan (tests/test_stream_deliver_host.py).  mib::stream_rounds -- the product's loop -- runs
// over a model device whose "launch" decodes up to the output limit plus a random overshoot, or
// to where the input ends; the copy kernel's walk is replayed on host memory.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "stream_rounds.h"

using namespace mib;

static uint64_t g_seed = 0xD1B54A32D192ED03ull;
static uint64_t rnd() {
  g_seed ^= g_seed << 13;
  g_seed ^= g_seed >> 7;
  g_seed ^= g_seed << 17;
  return g_seed;
}
static uint64_t below(uint64_t n) { return n ? rnd() % n : 0; }

#define CHECK(x)                                                       \
  do {                                                                 \
    if (!(x)) {                                                        \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #x); \
      exit(1);                                                         \
    }                                                                  \
  } while (0)

#include "stream_copy_walk.h"

// A model stream behind a real StreamSession: `total` bytes of output from 1 + ceil(total /
// ratio) + 1 bytes of input (a header byte, `ratio` output bytes per input byte, an end byte).
// An uncompressed block [raw_pos, raw_pos + raw_len) decodes whole or not at all.
struct Model {
  StreamSession s;
  uint64_t total = 0, ratio = 1, slack = 0;
  bool fixed_slack = false;           // every launch overshoots by `slack`, not by up to it
  uint64_t raw_pos = 0, raw_len = 0;
  uint64_t fed = 0, dropped = 0;      // input bytes that have arrived / that left the pending input's front
  uint64_t decoded = 0, given = 0;    // stream position of the checkpoint / bytes calls have handed out
  uint64_t launches = 0;
  // what the next launch reports instead of its own result (0: nothing)
  int fault_status = 0;
  int64_t fault_out_pos = 0;

  uint64_t in_total() const { return 1 + (total + ratio - 1) / ratio + 1; }
  uint64_t raw_needs() const { return 1 + (raw_pos + raw_len + ratio - 1) / ratio; }
  // the output position x bytes of input determine
  uint64_t out_of(uint64_t x) const {
    if (x >= in_total()) return total;
    uint64_t o = std::min(total, (x ? x - 1 : 0) * ratio);
    if (raw_len && o > raw_pos && o < raw_pos + raw_len) o = raw_pos;
    return o;
  }
  bool done() const { return s.finished && held(s) == 0 && !s.due; }
};

// The device of the model: decides nothing, fills StreamJob and the checkpoint head as
// decode_resume_kernel does, and checks what the rounds ask of it.
struct ModelDev {
  std::vector<Model *> m;
  std::vector<StreamSlot> *slots = nullptr;
  uint64_t input_moves = 0;
  bool launched = false;

  int launch(const std::vector<size_t> &jobs, const std::vector<StreamPlan> &plans, int final, StreamJob *ret, uint8_t *heads) {
    CHECK(!jobs.empty() && jobs.size() == plans.size());
    launched = true;
    for (size_t a = 0; a < jobs.size(); a++) {
      Model &md = *m[jobs[a]];
      StreamSession &s = md.s;
      const StreamSlot &slot = (*slots)[jobs[a]];
      const StreamPlan &p = plans[a];
      CHECK(a == 0 || jobs[a] > jobs[a - 1]);   // a slot has one job in a launch
      CHECK(!s.error && !slot.rc && !s.finished);
      CHECK(held(s) == 0 && slot.room > 0);     // a launch only with nothing held and room left
      CHECK(final || s.in_len >= s.need_len);   // never one that could only stop where the last did
      CHECK(md.dropped + s.in_len == md.fed);
      const uint64_t start = s.ck.e.pos;
      CHECK(s.deliv == start);
      CHECK(start <= (1ull << s.lgwin));        // the history has moved to the front
      CHECK(p.move + start <= s.buf_cap);       // the move's source lies in the buffer
      CHECK(p.out_limit > start && p.out_limit <= start + s.out_window);
      CHECK(p.out_limit - start <= slot.room);
      CHECK(p.out_limit + kStreamSlack <= s.buf_cap);
      // up to the first boundary at or behind out_limit (up to `slack` further), or to where the input ends
      const uint64_t left = md.out_of(md.fed) - md.decoded;
      uint64_t n = p.out_limit - start + (md.fixed_slack ? md.slack : below(md.slack + 1));
      StreamJob j;
      memset(&j, 0, sizeof(j));
      j.status = kStreamNeedOutput;
      if (n >= left) {
        n = left;
        j.status = md.fed >= md.in_total() ? kStreamFinished : kStreamNeedInput;
      }
      md.decoded += n;
      md.launches++;
      j.out_pos = (int64_t)(start + n);
      if (j.status == kStreamNeedInput) {
        j.redone = (int64_t)below(100);
        if (md.raw_len && md.decoded == md.raw_pos) j.need_len = (int64_t)(md.raw_needs() - md.dropped);
      }
      StreamCkpt ck = s.ck;
      const uint64_t used = j.status == kStreamFinished ? md.in_total() : std::min(md.fed, 1 + md.decoded / md.ratio);
      CHECK(used >= md.dropped);
      ck.e.pos = start + n;
      ck.e.bit = ck.e.mb_bit = 8 * (used - md.dropped);
      ck.e.flags = kPartValid | kPartAtMb;
      ck.win_off = (int64_t)((used - md.dropped) - below(std::min<uint64_t>(used - md.dropped, kStreamWin) + 1));
      if (md.fault_status) {
        j.status = md.fault_status;
        j.out_pos = md.fault_out_pos;
        md.fault_status = 0;
      }
      ret[a] = j;
      memcpy(heads + a * kStreamCkHead, &ck, kStreamCkHead);
    }
    return 0;
  }

  int deliver(std::vector<StreamSlot> &sl, const std::vector<size_t> &who, const std::vector<uint64_t> &len) {
    CHECK(who.size() == len.size());
    CHECK(!who.empty() || launched);   // a round without a job delivers
    launched = false;
    for (size_t g = 0; g < who.size(); g++) {
      Model &md = *m[who[g]];
      CHECK(!sl[who[g]].rc && len[g] > 0);
      CHECK(len[g] <= sl[who[g]].room && len[g] <= held(md.s));
      CHECK(md.given + held(md.s) == md.decoded);   // delivered + held is conserved
      md.given += len[g];
    }
    return 0;
  }

  int move_inputs(const std::vector<size_t> &who, const std::vector<uint64_t> &drop) {
    CHECK(!who.empty() && who.size() == drop.size());
    for (size_t g = 0; g < who.size(); g++) {
      Model &md = *m[who[g]];
      CHECK(drop[g] >= kStreamInputDropMin && drop[g] % 2 == 0);
      md.dropped += drop[g];
      CHECK(md.dropped + md.s.in_len == md.fed);   // (the session's length is already the moved one)
      CHECK(md.s.ck.win_off >= 0 && (md.s.ck.e.bit >> 3) <= md.s.in_len);
      input_moves++;
    }
    return 0;
  }
};

static uint64_t g_input_moves = 0;

// One call over k model sessions: slot i brings n[i] bytes (finish: none) and has room[i].  The
// host's part of the call is admission and the status; everything between is stream_rounds.
static void batch(const std::vector<Model *> &ms, const uint64_t *n, const uint64_t *room, bool finish, int *status,
                  uint64_t *given) {
  const size_t k = ms.size();
  std::vector<StreamSlot> slots(k);
  std::vector<uint64_t> before(k), had(k);
  ModelDev dev;
  dev.m = ms;
  dev.slots = &slots;
  bool device = false;
  for (size_t i = 0; i < k; i++) {
    Model &md = *ms[i];
    StreamSlot &slot = slots[i];
    slot.s = &md.s;
    slot.room = room[i];
    before[i] = md.launches;
    had[i] = md.given;
    const StreamAdmit a = stream_admit(md.s, finish ? 0 : n[i], finish);
    if (stream_admit_needs_device(a, md.s)) device = true;
    stream_admit_slot(slot, a);
    if (a != StreamAdmit::kFeed) continue;
    if (!md.s.lgwin) {   // (opened: a small window, so that the history moves often)
      md.s.lgwin = 10;
      md.s.buf_cap = stream_buf_cap(md.s.lgwin, md.s.out_window);
      stream_initial_ckpt(&md.s.ck, md.s.lgwin);
    }
    md.fed += finish ? 0 : n[i];
    md.s.in_len += finish ? 0 : n[i];   // (the chunk is appended)
    slot.run = true;
  }
  if (device) CHECK(stream_rounds(dev, slots, finish ? 1 : 0) == 0);
  g_input_moves += dev.input_moves;
  for (size_t i = 0; i < k; i++) {
    Model &md = *ms[i];
    const StreamSlot &slot = slots[i];
    given[i] = slot.given;
    CHECK(slot.given == md.given - had[i] && slot.given <= room[i]);
    CHECK(slot.room == room[i] - slot.given);
    if (room[i] == 0) CHECK(md.launches == before[i] && slot.given == 0);   // room 0: no launch
    if (md.s.error) {
      status[i] = md.s.error;
      CHECK(md.launches == before[i] && slot.given == 0);   // a failed session does nothing
      continue;
    }
    if (slot.rc) {
      status[i] = md.s.error = slot.rc;
      continue;
    }
    CHECK(md.given + held(md.s) == md.decoded);
    const bool more = stream_more_output(held(md.s), slot.room, md.s.due);
    // MORE_OUTPUT exactly when the range is full and work remains
    CHECK(more == (slot.given == room[i] && (held(md.s) > 0 || md.s.due)));
    if (!more) CHECK(held(md.s) == 0 && !md.s.due);
    status[i] = more ? 1 : 0;
    // status 0: everything the input determines has been delivered
    if (!more) CHECK(md.given == md.out_of(md.fed));
    if (!more && finish) CHECK(md.s.finished);
  }
}

static void random_model(Model &md) {
  md.total = below(3) == 0 ? below(50) : below(3 << 20);
  md.ratio = 1 + below(8);
  md.s.out_window = below(2) ? kStreamMinWindow : kStreamMinWindow + below(1 << 20);
  md.slack = below(3) == 0 ? 0 : below(2) ? below(300) : below(1 << 20);
  if (below(3) == 0 && md.total > 2) {
    md.raw_pos = below(md.total - 1);
    md.raw_len = 1 + below(std::min<uint64_t>(md.total - md.raw_pos, 1 << 18));
  }
}

// k sessions advanced together by random calls, each slot with a room of its own, until every
// stream is finished and handed out
static void drive(size_t k, int rounds) {
  const uint64_t rooms[] = {0, 1, 2, 15, 16, 17, 4097, 65536, 1 << 20, kNoRoomLimit};
  for (int r = 0; r < rounds; r++) {
    std::vector<Model> store(k);
    std::vector<Model *> ms;
    for (Model &md : store) {
      random_model(md);
      ms.push_back(&md);
    }
    std::vector<uint64_t> in(k), room(k), got(k);
    std::vector<int> st(k), idle(k, 0);
    auto all_done = [&] {
      for (const Model &md : store)
        if (!md.done()) return false;
      return true;
    };
    for (int step = 0; step < 100000 && !all_done(); step++) {
      bool whole = true;
      for (size_t i = 0; i < k; i++) {
        const Model &md = store[i];
        in[i] = md.fed < md.in_total() && below(4) ? 1 + below(md.in_total() / 3 + 2) : 0;
        in[i] = std::min(in[i], md.in_total() - md.fed);   // (trailing bytes have a case of their own)
        if (md.fed < md.in_total()) whole = false;
        room[i] = rooms[below(sizeof(rooms) / sizeof(rooms[0]))];
        if (idle[i] > 3) room[i] = 4097;   // (a run of empty ranges: let the session move)
      }
      // finish() once every stream's input is whole, as a caller does
      const bool finish = whole && below(2);
      std::vector<uint64_t> fed0(k);
      for (size_t i = 0; i < k; i++) fed0[i] = store[i].fed + (finish ? 0 : in[i]);
      batch(ms, in.data(), room.data(), finish, st.data(), got.data());
      for (size_t i = 0; i < k; i++) {
        CHECK(st[i] >= 0 && store[i].fed == fed0[i]);
        idle[i] = got[i] == 0 && (finish || in[i] == 0) ? idle[i] + 1 : 0;
      }
      // drain with empty chunks, as a caller does
      if (below(2))
        for (int q = 0; q < 1 << 22; q++) {
          bool more = false;
          for (size_t i = 0; i < k; i++) {
            in[i] = 0;
            room[i] = 1 + below(70000);
          }
          batch(ms, in.data(), room.data(), false, st.data(), got.data());
          for (size_t i = 0; i < k; i++)
            if (st[i] == 1) {
              CHECK(got[i] == room[i]);
              more = true;
            }
          if (!more) break;
        }
    }
    for (const Model &md : store) CHECK(md.done() && md.given == md.total && md.decoded == md.total);
  }
}

static void test_delivery(int rounds) {
  g_input_moves = 0;
  drive(1, rounds);
  CHECK(g_input_moves > 0);   // (the streams are long enough for their input to be compacted)
  printf("delivery ok\n");
}

// k = 3 slots with rooms of their own in one call
static void test_three_slots(int rounds) {
  drive(3, rounds);
  printf("three slots ok\n");
}

// one model, opened and fed `in` bytes with unlimited room
static int feed(Model &md, uint64_t in, uint64_t room, bool finish, uint64_t *given) {
  int st = 0;
  std::vector<Model *> ms{&md};
  batch(ms, &in, &room, finish, &st, given);
  return st;
}
static Model plain_model(uint64_t total) {
  Model md;
  md.total = total;
  md.ratio = 4;
  md.s.out_window = kStreamMinWindow;
  return md;
}

// every outcome of the accounting of a launch and of the admission to a call
static void test_outcomes() {
  uint64_t got = 0;
  {   // a negative status ends that slot and no other
    Model a = plain_model(1000), b = plain_model(1000), c = plain_model(1000);
    b.fault_status = -9;
    std::vector<Model *> ms{&a, &b, &c};
    uint64_t in[3] = {a.in_total(), b.in_total(), c.in_total()}, room[3] = {kNoRoomLimit, kNoRoomLimit, kNoRoomLimit}, g[3];
    int st[3];
    batch(ms, in, room, false, st, g);
    CHECK(st[0] == 0 && st[1] == -9 && st[2] == 0);
    CHECK(g[0] == 1000 && g[1] == 0 && g[2] == 1000 && a.s.finished && c.s.finished && !b.s.finished);
    CHECK(b.s.passes == 1 && b.s.total_out == 0);
    // ... and every later call of the failed session reports it without a launch
    in[0] = in[1] = in[2] = 0;
    batch(ms, in, room, true, st, g);
    CHECK(st[0] == 0 && st[1] == -9 && st[2] == 0 && b.launches == 1);
    CHECK(stream_admit(b.s, 5, false) == StreamAdmit::kNothing && !stream_admit_needs_device(StreamAdmit::kNothing, b.s));
  }
  for (int behind = 0; behind < 2; behind++) {   // out_pos in front of the launch's start, or behind the buffer
    Model a = plain_model(1000);
    a.fault_status = kStreamNeedInput;
    a.fault_out_pos = behind ? (int64_t)stream_buf_cap(10, kStreamMinWindow) + 1 : -1;
    CHECK(feed(a, 100, kNoRoomLimit, false, &got) == MIB_E_NO_PROGRESS && got == 0 && a.s.total_out == 0);
  }
  {   // total_out over max_out: MIB_E_OUTPUT_LIMIT, and none of the launch's bytes is held
    Model a = plain_model(1000);
    a.s.max_out = 399;
    CHECK(feed(a, 1 + 50, kNoRoomLimit, false, &got) == 0 && got == 200);
    CHECK(feed(a, 50, kNoRoomLimit, false, &got) == MIB_E_OUTPUT_LIMIT && got == 0);
    CHECK(held(a.s) == 0 && a.s.total_out == 400);
    Model b = plain_model(1000);   // (exactly the limit is allowed)
    b.s.max_out = 400;
    CHECK(feed(b, 1 + 100, kNoRoomLimit, false, &got) == 0 && got == 400);
  }
  {   // finished, with input behind the stream's end: -17
    Model a = plain_model(1000);
    CHECK(feed(a, a.in_total() + 1, kNoRoomLimit, false, &got) == -17 && a.s.finished);
  }
  {   // a finished session that still holds bytes: an empty chunk delivers them; a chunk is
      // refused (-17) and ends the session with what it holds
    Model a = plain_model(1000), b = plain_model(1000);
    a.slack = b.slack = 2000;   // (the first launch runs past its limit to the stream's end)
    a.fixed_slack = b.fixed_slack = true;
    CHECK(feed(a, a.in_total(), 300, false, &got) == 1 && got == 300 && a.s.finished && held(a.s) == 700);
    CHECK(stream_admit(a.s, 0, false) == StreamAdmit::kDeliver && stream_admit(a.s, 0, true) == StreamAdmit::kDeliver);
    CHECK(feed(a, 0, 500, false, &got) == 1 && got == 500);
    CHECK(feed(a, 0, 500, true, &got) == 0 && got == 200 && a.launches == 1);
    CHECK(stream_admit(a.s, 0, false) == StreamAdmit::kNothing && stream_admit(a.s, 0, true) == StreamAdmit::kNothing);
    CHECK(stream_admit(a.s, 1, false) == StreamAdmit::kTrailing && !stream_admit_needs_device(StreamAdmit::kTrailing, a.s));
    CHECK(feed(a, 1, 500, false, &got) == -17 && got == 0);
    CHECK(feed(b, b.in_total(), 300, false, &got) == 1 && held(b.s) == 700);
    CHECK(stream_admit(b.s, 1, false) == StreamAdmit::kTrailing && stream_admit_needs_device(StreamAdmit::kTrailing, b.s));
    CHECK(feed(b, 1, 500, false, &got) == -17 && got == 0 && b.launches == 1);
  }
  {   // NeedInput under `final`: the stream is cut short
    Model a = plain_model(1000);
    CHECK(feed(a, 100, kNoRoomLimit, false, &got) == 0 && got == 396 && !a.s.finished);
    CHECK(feed(a, 0, kNoRoomLimit, true, &got) == MIB_E_NO_PROGRESS && got == 0 && a.s.passes == 2);
  }
  {   // a launch owed from a call whose range ran out: kDue, and it launches without new input
    Model a = plain_model(200000);
    CHECK(feed(a, a.in_total(), kStreamMinWindow, false, &got) == 1 && got == kStreamMinWindow);
    while (held(a.s)) CHECK(feed(a, 0, 1000, false, &got) == 1);
    CHECK(a.s.due && stream_admit(a.s, 0, false) == StreamAdmit::kDue);
    const uint64_t l0 = a.launches;
    CHECK(feed(a, 0, 10, false, &got) == 1 && got == 10 && a.launches == l0 + 1);
  }
  {   // a session that has seen nothing: an empty update does nothing, finish() opens it
    Model a = plain_model(0);
    CHECK(stream_admit(a.s, 0, false) == StreamAdmit::kNothing && stream_admit(a.s, 0, true) == StreamAdmit::kFeed);
  }
  printf("outcomes ok\n");
}

// need_len keeps a session out of a call's first round until the bytes are there or finish() says
// that no more come
static void test_need_len() {
  uint64_t got = 0;
  for (int fin = 0; fin < 2; fin++) {
    Model a = plain_model(100000);
    a.raw_pos = 400;
    a.raw_len = 40000;
    CHECK(feed(a, 1 + 200, kNoRoomLimit, false, &got) == 0 && got == 400);
    CHECK(a.s.need_len == a.raw_needs() && a.s.need_len > a.s.in_len + 2);
    const uint64_t l0 = a.launches;
    CHECK(feed(a, 1, kNoRoomLimit, false, &got) == 0 && got == 0 && a.launches == l0);   // still short: no launch
    if (fin) {   // finish(): the launch is made, and finds the stream cut short
      CHECK(feed(a, 0, kNoRoomLimit, true, &got) == MIB_E_NO_PROGRESS && a.launches == l0 + 1);
    } else {
      CHECK(feed(a, a.raw_needs() - a.fed - 1, kNoRoomLimit, false, &got) == 0 && got == 0 && a.launches == l0);
      CHECK(feed(a, 1, kNoRoomLimit, false, &got) == 0 && got >= 40000 && a.launches > l0);
    }
  }
  printf("need_len ok\n");
}

// the rule for compacting the pending input: at least 64 KiB leave, and at least half
static void test_input_compaction() {
  const uint64_t k64 = 64u << 10;
  struct Case { uint64_t keep, in_len, need_len, drop; };
  const Case cases[] = {
      {k64 - 2, k64 - 2, 0, 0},              {k64 - 2, 2 * (k64 - 2), 0, 0},   // below 64 KiB: never
      {k64, 2 * k64 + 1, 0, 0},              {k64, 2 * k64, 0, k64},           // 2 * keep just below / at in_len
      {k64, k64, 0, k64},                    {k64 + 2, 2 * k64 + 5, 0, 0},
      {k64 + 2, 2 * k64 + 4, k64 + 9, k64 + 2},                                // need_len moves down with the input
      {k64 + 2, 2 * k64 + 4, k64 + 2, k64 + 2}, {k64 + 2, 2 * k64 + 4, 7, k64 + 2},   // ... and not below 0
  };
  for (const Case &c : cases) {
    StreamSession s;
    stream_initial_ckpt(&s.ck, 16);
    s.ck.e.bit = s.ck.e.mb_bit = 8 * c.keep + 3;
    s.ck.win_off = (int64_t)c.keep + 1;   // (keep is even: the odd byte stays)
    s.in_len = c.in_len;
    s.need_len = c.need_len;
    CHECK(stream_keep_from(s.ck) == c.keep);
    CHECK(stream_compact_input(s) == c.drop);
    CHECK(s.in_len == c.in_len - c.drop);
    CHECK(s.need_len == (c.need_len > c.drop ? c.need_len - c.drop : 0));
    CHECK(s.ck.e.bit == 8 * (c.keep - c.drop) + 3 && s.ck.win_off == (int64_t)(c.keep - c.drop) + 1);
  }
  printf("input compaction ok\n");
}

// the host call's slot: no limit, so every round's bytes are delivered whole and nothing is
// ever held or owed behind the call -- the planning reduces to what the host path always did
static void test_host_slot(int rounds) {
  for (int r = 0; r < rounds; r++) {
    const uint64_t start = below(1ull << 29), w = kStreamMinWindow + below(kStreamMaxWindow - kStreamMinWindow);
    CHECK(stream_out_limit(start, w, kNoRoomLimit) == start + w);
    const uint64_t h = below(1ull << 30);
    CHECK(deliver_len(h, kNoRoomLimit) == h);
    CHECK(!stream_more_output(h, kNoRoomLimit - h, true));
    CHECK(stream_plans_job(0, kNoRoomLimit, true) && !stream_plans_job(h + 1, kNoRoomLimit, true) &&
          !stream_plans_job(0, kNoRoomLimit, false) && !stream_plans_job(0, 0, true));
  }
  printf("host slot ok\n");
}

// the copy launches replayed on host memory (stream_copy_walk.h): each destination byte must be
// written exactly once, with its source byte, and nothing outside the destinations.  Destinations are packed with random gaps from 0,
// so neighbours share 16-byte granules.
static void test_copies(int rounds) {
  for (int r = 0; r < rounds; r++) {
    const size_t k = 1 + below(40);
    const size_t max_descs = 1 + below(r % 3 == 0 ? 3 : 50);
    std::vector<uint64_t> n(k), at(k), sat(k);
    uint64_t dtotal = below(16), stotal = below(16);
    for (size_t i = 0; i < k; i++) {
      const uint64_t pick = below(8);
      n[i] = pick == 0 ? 0 : pick == 1 ? 1 : pick < 5 ? below(70) : pick < 7 ? below(3 * kGatherTile) : kGatherTile * (1 + below(3)) + below(3) - 1;
      if (r % 50 == 7 && i == 0) n[i] = (kGatherSpread + 1) * kGatherTile + 17;   // more tiles than blocks
      at[i] = dtotal;
      dtotal += n[i] + (below(2) ? 0 : below(20));
      sat[i] = stotal;
      stotal += n[i] + below(20);
    }
    // 16-byte aligned bases, as device allocations are
    std::vector<uint8_t> dmem(dtotal + 48), smem(stotal + 48), cnt(dtotal + 48, 0);
    uint8_t *db = dmem.data() + ((16 - ((uintptr_t)dmem.data() & 15)) & 15);
    uint8_t *sb = smem.data() + ((16 - ((uintptr_t)smem.data() & 15)) & 15);
    for (size_t q = 0; q < smem.size(); q++) smem[q] = (uint8_t)rnd();
    memset(dmem.data(), 0xC5, dmem.size());
    std::vector<CopyDesc> d(k);
    for (size_t i = 0; i < k; i++) d[i] = CopyDesc{sb + sat[i], db + at[i], n[i]};
    std::vector<CopyLaunch> ls;
    plan_copies(d.data(), k, max_descs, ls);
    // the split covers every descriptor once, in order
    size_t next = 0;
    for (const CopyLaunch &l : ls) {
      CHECK(l.first == next && l.count >= 1 && l.count <= max_descs);
      CHECK(l.blocks >= 1 && l.blocks <= kGatherSpread);
      CHECK(l.blocks == copy_blocks(d.data() + l.first, l.count));
      next += l.count;
    }
    CHECK(next == k);
    replay_copies(d.data(), ls, dmem.data(), cnt);
    std::vector<uint8_t> want(dmem.size(), 0xC5), wcnt(dmem.size(), 0);
    for (size_t i = 0; i < k; i++)
      for (uint64_t q = 0; q < n[i]; q++) {
        want[(size_t)(db + at[i] + q - dmem.data())] = sb[sat[i] + q];
        wcnt[(size_t)(db + at[i] + q - dmem.data())] = 1;
      }
    CHECK(dmem == want);
    CHECK(cnt == wcnt);
  }
  printf("copies ok\n");
}

int main() {
  test_delivery(400);
  test_three_slots(150);
  test_outcomes();
  test_need_len();
  test_input_compaction();
  test_host_slot(2000);
  test_copies(150);
  return 0;
}
