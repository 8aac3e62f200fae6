// The tickets of the ticketed handles (hipfeat_mixer, hipfeat_reverb, hipfeat_level, hipfeat_collate, hipfeat_sinc, hipfeat_featmix): a plan hands out
// a ticket, a run consumes it.  Up to kTicketSlots plans may be outstanding; ticket t lives in slot t % kTicketSlots, and a plan is
// refused while the slot its ticket would take still holds one that has not run.
// Pure C++ (no HIP): also compiled by tests/native/collate_tables_capi.cpp and checked on the CPU (tests/test_collate_abi.py).
#pragma once
#include <cstdint>

namespace hipfeat {

constexpr int kTicketSlots = 16;

struct TicketRing {
  int64_t ticket[kTicketSlots];
  bool planned[kTicketSlots];
  int64_t next_ticket = 0;
  TicketRing() {
    for (int i = 0; i < kTicketSlots; ++i) ticket[i] = -1, planned[i] = false;
  }
  bool full() const { return planned[next_ticket % kTicketSlots]; }
  int64_t take() {  // -> the new ticket, or -1 when kTicketSlots plans are outstanding
    if (full()) return -1;
    const int64_t t = next_ticket++;
    ticket[t % kTicketSlots] = t;
    planned[t % kTicketSlots] = true;
    return t;
  }
  int slot_of(int64_t t) const {  // -> the slot of a planned ticket, or -1
    const int i = (int)(((t % kTicketSlots) + kTicketSlots) % kTicketSlots);
    return ticket[i] == t && planned[i] ? i : -1;
  }
  bool release(int64_t t) {
    const int i = slot_of(t);
    if (i >= 0) planned[i] = false;
    return i >= 0;
  }
};

}  // namespace hipfeat
