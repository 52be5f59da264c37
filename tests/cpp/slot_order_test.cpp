// slot_order_test.cpp — the ticket order of zkemail.rs_amd/csrc/slot_order.hip.h, walked on the CPU.
//
// For every slot count 1 .. 64, every split of the slots into 1 .. 8 groups whose sizes differ by at most 2 (each in three placements of
// the groups over the slot indices: dealt out in turn, in blocks, shuffled), and the splits HIP's queue pool really produces (6/6/5/5,
// 5/5/4/4, 4/4/4/4) plus an uneven 7/1:
//   * an unknown map (a probe word missing, more groups than queues) and all-singleton groups give t % slots for every t;
//   * any n_queues consecutive tickets hit every queue once;
//   * a queue's slots come round in ascending order, each once per count[q] visits;
//   * every slot is used within n_queues x max count tickets;
//   * all of it holds across 2^32, where a 32-bit ticket counter would wrap.
// Stand-alone, built with -fsanitize=address,undefined by tests/test_slot_order.py.  Prints "slot_order_test ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../zkemail.rs_amd/csrc/slot_order.hip.h"

using namespace zke;

static uint64_t g_checked = 0;
#define REQUIRE(c, ...) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n  ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static uint32_t rng_state = 12345;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// the ids a probe would report: group g of a slot -> an arbitrary distinct word
static uint32_t id_of_group(uint32_t g) { return 0x40000040u + (g << 24) + ((g & 3u) << 6) + 0x1000u * g; }

// t % slots over windows at 0, below and across 2^32, and far above it
static const uint64_t STARTS[] = {0, (1ull << 32) - 700, (1ull << 40) + 12345};

static void check_round_robin(const SlotOrder& o, uint32_t slots) {
  REQUIRE(o.n_queues == 0 && o.slots == slots, "slots %u", slots);
  for (uint64_t start : STARTS)
    for (uint64_t t = start; t < start + 1400; t++) REQUIRE(slot_for_ticket(o, t) == t % slots, "slots %u ticket %llu", slots, (unsigned long long)t);
  for (uint32_t s = 0; s < slots; s++) REQUIRE(o.queue_of[s] == -1, "slot %u", s);
}

// group_of[s] for s < slots: any labelling with nq distinct labels 0 .. nq-1 (not yet in order of first sighting)
static void check_split(const std::vector<uint32_t>& group_of, uint32_t nq) {
  const uint32_t slots = (uint32_t)group_of.size();
  std::vector<uint32_t> id(slots);
  std::vector<uint8_t> known(slots, 1);
  for (uint32_t s = 0; s < slots; s++) id[s] = id_of_group(group_of[s]);
  SlotOrder o;
  const bool ok = slot_order_build(o, id.data(), known.data(), slots, nq);
  g_checked++;
  if (nq == slots) {          // a queue per slot: nothing to balance, exactly the order before there was a map
    REQUIRE(!ok, "slots %u", slots);
    check_round_robin(o, slots);
    return;
  }
  REQUIRE(ok && o.n_queues == nq && o.slots == slots, "slots %u nq %u", slots, nq);
  // the map: same group <=> same label; groups numbered by their lowest slot; lists ascending, disjoint, covering
  std::vector<uint32_t> seen_slot(slots, 0);
  uint32_t max_count = 0, lowest_prev = 0;
  for (uint32_t q = 0; q < nq; q++) {
    REQUIRE(o.count[q] >= 1, "queue %u empty", q);
    max_count = std::max<uint32_t>(max_count, o.count[q]);
    for (uint32_t k = 0; k < o.count[q]; k++) {
      const uint32_t s = o.list[o.first[q] + k];
      REQUIRE(s < slots && !seen_slot[s]++ && o.queue_of[s] == (int)q, "queue %u entry %u", q, k);
      if (k) REQUIRE(s > o.list[o.first[q] + k - 1], "queue %u not ascending", q);
      REQUIRE(group_of[s] == group_of[o.list[o.first[q]]], "queue %u mixes groups", q);
    }
    if (q) REQUIRE(o.list[o.first[q]] > lowest_prev, "queue %u out of order", q);
    lowest_prev = o.list[o.first[q]];
  }
  for (uint32_t s = 0; s < slots; s++) REQUIRE(seen_slot[s] == 1, "slot %u", s);
  for (uint32_t a = 0; a < slots; a++)
    for (uint32_t b = 0; b < slots; b++) REQUIRE((group_of[a] == group_of[b]) == (o.queue_of[a] == o.queue_of[b]), "slots %u %u", a, b);

  const uint32_t reach = nq * max_count;
  for (uint64_t start : STARTS) {
    const uint32_t len = 3 * reach + 1400;
    std::vector<uint32_t> seq(len);
    for (uint32_t i = 0; i < len; i++) { seq[i] = slot_for_ticket(o, start + i); REQUIRE(seq[i] < slots, "ticket %u", i); }
    // any n_queues consecutive tickets hit every queue once: ticket t is on queue t % n_queues
    for (uint32_t i = 0; i < len; i++) REQUIRE((uint32_t)o.queue_of[seq[i]] == (start + i) % nq, "ticket %llu", (unsigned long long)(start + i));
    // a queue's visits take its slots in ascending order, each once per count[q] visits — also across 2^32
    std::vector<int> prev_pos(nq, -1);
    for (uint32_t i = 0; i < len; i++) {
      const uint32_t q = (uint32_t)o.queue_of[seq[i]];
      int pos = -1;
      for (uint32_t k = 0; k < o.count[q]; k++) if (o.list[o.first[q] + k] == seq[i]) pos = (int)k;
      if (prev_pos[q] >= 0) REQUIRE(pos == (prev_pos[q] + 1) % (int)o.count[q], "queue %u ticket %llu", q, (unsigned long long)(start + i));
      prev_pos[q] = pos;
    }
    // every slot within n_queues x max count tickets, from wherever the window starts
    std::vector<uint32_t> last(slots, 0);
    std::vector<uint8_t> ever(slots, 0);
    for (uint32_t i = 0; i < len; i++) {
      if (ever[seq[i]]) REQUIRE(i - last[seq[i]] <= reach, "slot %u waited %u tickets", seq[i], i - last[seq[i]]);
      else REQUIRE(i < reach, "slot %u first used at %u", seq[i], i);
      ever[seq[i]] = 1; last[seq[i]] = i;
    }
  }

  // the map counts as unknown: a probe word that was not written, more groups than the pool has queues
  known[rng() % slots] = 0;
  REQUIRE(!slot_order_build(o, id.data(), known.data(), slots, nq), "unwritten word");
  check_round_robin(o, slots);
  known.assign(slots, 1);
  if (nq > 1) {
    REQUIRE(!slot_order_build(o, id.data(), known.data(), slots, nq - 1), "more groups than queues");
    check_round_robin(o, slots);
  }
}

// sizes -> three placements of the groups over the slot indices
static void check_sizes(const std::vector<uint32_t>& sizes) {
  const uint32_t nq = (uint32_t)sizes.size();
  uint32_t slots = 0;
  for (uint32_t c : sizes) slots += c;
  std::vector<uint32_t> dealt, blocks;
  std::vector<uint32_t> left = sizes;
  for (uint32_t q = 0; dealt.size() < slots; q = (q + 1) % nq) if (left[q]) { left[q]--; dealt.push_back(q); }      // what a runtime that fills the emptiest queue does
  for (uint32_t q = 0; q < nq; q++) blocks.insert(blocks.end(), sizes[q], q);
  std::vector<uint32_t> shuffled = blocks;
  for (uint32_t i = slots; i > 1; i--) std::swap(shuffled[i - 1], shuffled[rng() % i]);
  check_split(dealt, nq);
  check_split(blocks, nq);
  check_split(shuffled, nq);
}

// every non-increasing tuple of nq sizes with sum `slots` and max - min <= 2
static void enumerate(uint32_t nq, std::vector<uint32_t>& sizes, uint32_t left, uint32_t hi, uint32_t top) {
  if (sizes.size() == nq) { if (left == 0) check_sizes(sizes); return; }
  for (uint32_t c = std::min(hi, left); c >= 1; c--) {
    if (top && top - c > 2) break;
    sizes.push_back(c);
    enumerate(nq, sizes, left - c, c, top ? top : c);
    sizes.pop_back();
  }
}

int main() {
  for (uint32_t slots = 1; slots <= 64; slots++) {
    SlotOrder o;
    slot_order_unknown(o, slots);
    check_round_robin(o, slots);
    for (uint32_t nq = 1; nq <= 8 && nq <= slots; nq++) {
      std::vector<uint32_t> sizes;
      enumerate(nq, sizes, slots, slots, 0);
    }
    std::vector<uint32_t> singles(slots);          // all-singleton groups, more than eight of them too
    for (uint32_t s = 0; s < slots; s++) singles[s] = s;
    check_split(singles, slots);
  }
  check_sizes({6, 6, 5, 5});
  check_sizes({5, 5, 4, 4});
  check_sizes({4, 4, 4, 4});
  check_sizes({7, 1});
  check_sizes({1, 7});
  // 6 / 6 / 5 / 5 as the runtime deals 22 streams: the shares are 1/4 each, the step no longer 6/22
  {
    std::vector<uint32_t> g(22);
    for (uint32_t s = 0; s < 22; s++) g[s] = s % 4;
    std::vector<uint32_t> id(22);
    std::vector<uint8_t> known(22, 1);
    for (uint32_t s = 0; s < 22; s++) id[s] = id_of_group(g[s]);
    SlotOrder o;
    REQUIRE(slot_order_build(o, id.data(), known.data(), 22, 4), "22 on 4");
    uint32_t per_queue[4] = {};
    for (uint64_t t = 0; t < 120; t++) per_queue[(uint32_t)o.queue_of[slot_for_ticket(o, t)]]++;
    for (uint32_t q = 0; q < 4; q++) REQUIRE(per_queue[q] == 30, "queue %u took %u of 120", q, per_queue[q]);
    REQUIRE(slot_for_ticket(o, 0) == 0 && slot_for_ticket(o, 1) == 1 && slot_for_ticket(o, 4) == 4 && slot_for_ticket(o, 20) == 20 &&
            slot_for_ticket(o, 21) == 21 && slot_for_ticket(o, 22) == 2 && slot_for_ticket(o, 23) == 3 && slot_for_ticket(o, 24) == 0, "first tickets");
  }
  printf("slot_order_test ok: %llu maps\n", (unsigned long long)g_checked);
  return 0;
}
