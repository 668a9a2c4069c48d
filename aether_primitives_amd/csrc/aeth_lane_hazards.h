// aeth_lane_hazards.h -- which launches of the overlap lane (aeth_ctx_set_overlap) may run beside each other, decided
// on the host from the byte ranges they touch.  Free of HIP types and calls, like aeth_hostcore.h, so that it also builds
// with plain g++ under -fsanitize=address,undefined (tests/cpp/lane_hazards_sanitize.cpp, driven by
// tests/test_lane_hazards_host.py).
//
// The two lanes are in-order queues: a launch is ordered behind every earlier launch of ITS lane by the queue itself.
// What the queue does not order is the other lane, so the tracker keeps, per lane, the ranges of the launches enqueued
// there since the last join (a point at which one queue was made to wait for the other), and answers one question: does
// a new launch read what a launch of that lane writes (read-after-write), write what it reads (write-after-read) or
// write what it writes (write-after-write)?  Nothing is ever known to have FINISHED without a join, so records leave
// only by reset().
#pragma once

#include <cstddef>
#include <cstdint>

namespace aeth {
namespace lanes {

// [lo, hi) in bytes; lo >= hi is the empty range and touches nothing
struct Range {
    uintptr_t lo = 0, hi = 0;
    bool empty() const { return lo >= hi; }
    bool operator==(const Range &o) const { return (empty() && o.empty()) || (lo == o.lo && hi == o.hi); }
};
inline Range range_of(const void *p, size_t bytes) { return Range{(uintptr_t)p, (uintptr_t)p + (p ? bytes : 0)}; }
inline bool touch(const Range &a, const Range &b) { return !a.empty() && !b.empty() && a.lo < b.hi && b.lo < a.hi; }

// everything one launch reads and writes
struct Access {
    Range in[2];
    Range out;
    bool operator==(const Access &o) const { return in[0] == o.in[0] && in[1] == o.in[1] && out == o.out; }
};

enum : unsigned { RAW = 1, WAR = 2, WAW = 4 };
// the hazards of launching `next` while `prev` may still run
inline unsigned hazards(const Access &next, const Access &prev)
{
    unsigned h = 0;
    for (int i = 0; i < 2; i++) {
        if (touch(next.in[i], prev.out)) h |= RAW;
        if (touch(next.out, prev.in[i])) h |= WAR;
    }
    if (touch(next.out, prev.out)) h |= WAW;
    return h;
}

class Tracker {
public:
    // Records per lane.  A stream processor rotates over a handful of buffer pairs (the benchmark over six, the host
    // pipeline over its device slots) and a launch whose ranges equal a record's takes no new slot, so such a chain holds
    // as many records as it has buffer pairs, however long it runs; 32 leaves room for any rotation that fits a device
    // at sizes where overlap pays, and a query still is at most 32 x 5 range compares, far below a launch's host cost.
    // A chain over more DISTINCT buffers than that pays one join per 32 launches of a lane.
    static constexpr int kSlots = 32;

    void reset() { n_[0] = n_[1] = 0; }
    int size(int lane) const { return n_[lane]; }

    // RAW | WAR | WAW of `a` against every record of `lane`; 0 = may run beside all of them
    unsigned hazards(int lane, const Access &a) const
    {
        unsigned h = 0;
        for (int i = 0; i < n_[lane]; i++) h |= lanes::hazards(a, rec_[lane][i]);
        return h;
    }
    // Enter a launch of `lane`.  Equal ranges refresh the record that holds them.  false: every slot is taken by
    // other ranges -- nothing was entered and nothing dropped; the caller joins the lanes and calls reset().
    bool note(int lane, const Access &a)
    {
        for (int i = 0; i < n_[lane]; i++)
            if (rec_[lane][i] == a) return true;
        if (n_[lane] == kSlots) return false;
        rec_[lane][n_[lane]++] = a;
        return true;
    }

private:
    Access rec_[2][kSlots];
    int n_[2] = {0, 0};
};

}  // namespace lanes
}  // namespace aeth
