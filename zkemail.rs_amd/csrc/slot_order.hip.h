// slot_order.hip.h — the order in which submission tickets visit the engine's slots.
//
// Every slot has a stream of its own, and HIP places the streams on the hardware queues of its pool: 22 streams on four queues sit
// 6 / 6 / 5 / 5.  A queue runs its kernels one after the other, so where the engine is chain-bound (DESIGN.md §5 "Hardware queues") its
// throughput is the fullest queue's share of the batches.  Tickets taken round-robin over the SLOTS hand a queue 6/22 or 5/22 of the batches;
// taken round-robin over the QUEUES, and over a queue's slots within it, every queue gets 1/n_queues.  Which slots share a queue is read from
// the device (pipeline.hip.h, slot_queue_probe_kernel); this file is the policy on plain integers.  Plain C++: no HIP runtime, no engine —
// tests/cpp/slot_order_test.cpp walks it on the CPU.
#pragma once
#include <stdint.h>

namespace zke {

constexpr uint32_t SLOT_ORDER_MAX_SLOTS = 64;      // zke_engine_reserve's bound

struct SlotOrder {
  uint32_t slots = 0;                            // slots the order covers (= the engine's, once built)
  uint32_t n_queues = 0;                         // groups of slots that share a hardware queue; 0: the map is unknown — plain t % slots
  int8_t queue_of[SLOT_ORDER_MAX_SLOTS];         // slot -> group, -1 unknown.  Groups are numbered in order of their lowest slot index
  uint8_t count[SLOT_ORDER_MAX_SLOTS];           // group -> how many slots it has
  uint8_t first[SLOT_ORDER_MAX_SLOTS];           // group -> where its slots start in `list`
  uint8_t list[SLOT_ORDER_MAX_SLOTS];            // the slots group by group, ascending within a group
};

inline void slot_order_unknown(SlotOrder& o, uint32_t slots) {
  o.slots = slots;
  o.n_queues = 0;
  for (uint32_t i = 0; i < SLOT_ORDER_MAX_SLOTS; i++) { o.queue_of[i] = -1; o.count[i] = 0; o.first[i] = 0; o.list[i] = 0; }
}

// The order from what the probe read: id[s] names the hardware queue slot s's stream sits on (any value; equal ids = same queue),
// known[s] == 0: the slot's probe word was not written.  The map counts as unknown — and the order is plain round-robin — when a
// slot is not known, when there are more distinct ids than the queue pool has queues (the ids then name something else), and when
// every slot has a queue to itself (nothing to balance: exactly t % slots, as before).  Returns whether the map is known.
inline bool slot_order_build(SlotOrder& o, const uint32_t* id, const uint8_t* known, uint32_t slots, uint32_t hw_queues) {
  slot_order_unknown(o, slots);
  if (slots == 0 || slots > SLOT_ORDER_MAX_SLOTS) return false;
  uint32_t group_id[SLOT_ORDER_MAX_SLOTS];
  int8_t queue_of[SLOT_ORDER_MAX_SLOTS];
  uint32_t nq = 0;
  for (uint32_t s = 0; s < slots; s++) {
    if (!known[s]) return false;
    uint32_t q = 0;
    while (q < nq && group_id[q] != id[s]) q++;
    if (q == nq) group_id[nq++] = id[s];          // first sighting, at the group's lowest slot index: groups are numbered in that order
    queue_of[s] = (int8_t)q;
  }
  if (nq > hw_queues || nq == slots) return false;
  o.n_queues = nq;
  for (uint32_t s = 0; s < slots; s++) { o.queue_of[s] = queue_of[s]; o.count[queue_of[s]]++; }
  uint32_t at = 0;
  for (uint32_t q = 0; q < nq; q++) { o.first[q] = (uint8_t)at; at += o.count[q]; }
  uint8_t fill[SLOT_ORDER_MAX_SLOTS] = {};
  for (uint32_t s = 0; s < slots; s++) { const uint32_t q = (uint32_t)queue_of[s]; o.list[o.first[q] + fill[q]++] = (uint8_t)s; }
  return true;
}

// Ticket t's slot: queue t % n_queues, and of that queue's slots the next in turn.  The tickets are 64 bits wide, so t % n_queues
// never meets a wrap.  With the map unknown this is t % slots, the order before there was a map.
inline uint32_t slot_for_ticket(const SlotOrder& o, uint64_t t) {
  if (o.n_queues == 0) return (uint32_t)(t % o.slots);
  const uint32_t q = (uint32_t)(t % o.n_queues);
  const uint64_t r = t / o.n_queues;
  return o.list[o.first[q] + (uint32_t)(r % o.count[q])];
}

}  // namespace zke
