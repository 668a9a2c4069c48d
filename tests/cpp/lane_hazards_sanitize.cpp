// lane_hazards_sanitize.cpp -- the overlap lane's hazard tracker (csrc/aeth_lane_hazards.h), exactly the code
// libaether_hip.so runs, on the CPU under the address and undefined-behaviour sanitizers.  Built and run by
// tests/test_lane_hazards_host.py:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I aether_primitives_amd/csrc ...
// Exit code 0 and "lane_hazards: ok" = every check passed and the sanitizers stayed silent.
#include "aeth_lane_hazards.h"

#include <cstdio>
#include <cstdlib>

using namespace aeth::lanes;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "lane_hazards: CHECK failed at line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

// a launch reading [in, in + n) (and [in2, in2 + n2)) and writing [out, out + n)
static Access acc(uintptr_t in, uintptr_t out, uintptr_t n, uintptr_t in2 = 0, uintptr_t n2 = 0)
{
    Access a;
    a.in[0] = Range{in, in + n};
    a.in[1] = Range{in2, in2 + n2};
    a.out = Range{out, out + n};
    return a;
}

int main()
{
    // ---- ranges: half-open, empty ones touch nothing
    CHECK(touch(Range{0, 10}, Range{9, 20}) && !touch(Range{0, 10}, Range{10, 20}) && !touch(Range{10, 20}, Range{0, 10}));
    CHECK(!touch(Range{5, 5}, Range{0, 10}) && !touch(Range{0, 10}, Range{}) && !touch(Range{}, Range{}));
    CHECK(range_of(nullptr, 64).empty() && range_of((const void *)0x1000, 0).empty());
    CHECK(range_of((const void *)0x1000, 64).lo == 0x1000 && range_of((const void *)0x1000, 64).hi == 0x1040);

    // ---- the three kinds, each alone, against one record a -> b on lane 0
    const uintptr_t A = 0x10000, B = 0x20000, C_ = 0x30000, D = 0x40000, S = 0x50000, N = 0x1000;
    {
        Tracker t;
        CHECK(t.size(0) == 0 && t.size(1) == 0 && t.hazards(0, acc(A, B, N)) == 0);
        CHECK(t.note(0, acc(A, B, N)) && t.size(0) == 1 && t.size(1) == 0);
        CHECK(t.hazards(0, acc(B, C_, N)) == RAW);                  // reads what the record writes
        CHECK(t.hazards(0, acc(C_, A, N)) == WAR);                  // writes what the record reads
        CHECK(t.hazards(0, acc(C_, B, N)) == WAW);                  // writes what the record writes
        CHECK(t.hazards(0, acc(B, A, N)) == (RAW | WAR));
        CHECK(t.hazards(0, acc(A, C_, N)) == 0);                    // two readers of one buffer
        CHECK(t.hazards(0, acc(C_, D, N)) == 0);
        CHECK(t.hazards(1, acc(B, A, N)) == 0);                     // the other lane holds nothing
        // one byte is enough, at either end
        CHECK(t.hazards(0, acc(B + N - 1, C_, N)) == RAW && t.hazards(0, acc(B - N + 1, C_, N)) == RAW);
        CHECK(t.hazards(0, acc(C_, B + N - 1, N)) == WAW && t.hazards(0, acc(C_, A - N + 1, N)) == WAR);
        // touching but not overlapping: the neighbour starts where the record ends, or ends where it starts
        CHECK(t.hazards(0, acc(B + N, C_, N)) == 0 && t.hazards(0, acc(B - N, C_, N)) == 0);
        CHECK(t.hazards(0, acc(C_, B + N, N)) == 0 && t.hazards(0, acc(C_, A - N, N)) == 0 && t.hazards(0, acc(C_, A + N, N)) == 0);
    }
    // ---- the second input: a record that reads S forbids a write of S, and a launch that reads S sees a writer of S
    {
        Tracker t;
        CHECK(t.note(1, acc(A, B, N, S, 64)));
        CHECK(t.hazards(1, acc(C_, S, 64)) == WAR && t.hazards(1, acc(C_, S + 64, 64)) == 0);
        CHECK(t.hazards(1, acc(S, C_, 64)) == 0);
        CHECK(t.note(0, acc(C_, S, 64)));
        CHECK(t.hazards(0, acc(A, D, N, S, 64)) == RAW && t.hazards(0, acc(A, D, N)) == 0);
    }
    // ---- hazards are found on any record of the lane, not only the latest
    {
        Tracker t;
        CHECK(t.note(0, acc(A, B, N)) && t.note(1, acc(C_, D, N)) && t.note(0, acc(0x60000, 0x70000, N)));
        CHECK(t.hazards(0, acc(B, 0x80000, N)) == RAW && t.hazards(1, acc(B, 0x80000, N)) == 0);
        CHECK(t.hazards(1, acc(0x80000, D, N)) == WAW && t.hazards(0, acc(0x80000, D, N)) == 0);
    }
    // ---- an equal record is refreshed, not entered again: a rotating buffer set never fills the lane
    {
        Tracker t;
        for (int rep = 0; rep < 1000; rep++)
            for (uintptr_t k = 0; k < 3; k++) CHECK(t.note(rep & 1, acc(A + k * 0x100000, B + k * 0x100000, N)));
        CHECK(t.size(0) == 3 && t.size(1) == 3);
        CHECK(t.note(0, acc(A, B, N - 1)) && t.size(0) == 4);       // other ranges: another record
        CHECK(t.note(0, acc(A, B, N, S, 8)) && t.size(0) == 5);
    }
    // ---- a full lane reports "join": nothing is entered, nothing is dropped, the other lane is untouched
    {
        Tracker t;
        for (int k = 0; k < Tracker::kSlots; k++) CHECK(t.note(0, acc(A + (uintptr_t)k * 0x100000, A + (uintptr_t)k * 0x100000 + 0x80000, N)));
        CHECK(t.size(0) == Tracker::kSlots);
        CHECK(!t.note(0, acc(0x9000000, 0x9100000, N)) && t.size(0) == Tracker::kSlots);
        CHECK(t.hazards(0, acc(A + 0x80000, 0x9000000, N)) == RAW);                                  // the oldest record is still there
        CHECK(t.hazards(0, acc(0x9000000, A + (uintptr_t)(Tracker::kSlots - 1) * 0x100000, N)) == WAR);   // and the newest
        CHECK(t.note(0, acc(A, A + 0x80000, N)));                                                     // a refresh still fits
        CHECK(t.note(1, acc(0x9000000, 0x9100000, N)) && t.size(1) == 1);
        // ---- reset: both lanes empty, everything fits again
        t.reset();
        CHECK(t.size(0) == 0 && t.size(1) == 0 && t.hazards(0, acc(A + 0x80000, 0x9000000, N)) == 0 && t.hazards(1, acc(0x9100000, D, N)) == 0);
        CHECK(t.note(0, acc(0x9000000, 0x9100000, N)) && t.size(0) == 1);
    }
    // ---- ranges at the top of the address space do not wrap into a match
    {
        Tracker t;
        const uintptr_t top = ~(uintptr_t)0;
        Access a; a.in[0] = Range{top - 64, top}; a.out = Range{top - 128, top - 64};
        CHECK(t.note(0, a) && t.hazards(0, acc(A, B, N)) == 0);
        Access b; b.in[0] = Range{top - 65, top - 64}; b.out = Range{B, B + N};
        CHECK(t.hazards(0, b) == RAW);
    }
    printf("lane_hazards: ok\n");
    return 0;
}
