// sqy_lanes.hpp -- which parse lane a call in flight takes (host only, no HIP: tests/sanitize/lane_picker_test.cpp builds it with g++).
//
// The library's lanes are streams of its own, per device (sqy_capi.cpp: one transpose lane, `parse_lanes` parse lanes).  A call leases
// the parse lane with the fewest calls leased to it; among equals the lanes take turns (round robin), so that calls which come and go
// one at a time still spread over all lanes -- and with them over the hardware queues behind them.  Not thread safe: the owner holds
// the device's lane mutex around take() and give().
#pragma once

namespace sqy {

class LanePicker {
public:
    static constexpr int kMaxLanes = 8;

    // leases one of the lanes 0 .. lanes-1 (lanes clamped to [1, kMaxLanes]) and says which
    int take(int lanes)
    {
        if (lanes < 1) lanes = 1;
        if (lanes > kMaxLanes) lanes = kMaxLanes;
        int best = -1;
        for (int k = 0; k < lanes; ++k) {
            const int i = (next_ + k) % lanes;              // (ties: the first lane at or behind the one whose turn it is)
            if (best < 0 || leased_[i] < leased_[best]) best = i;
        }
        leased_[best] += 1;
        next_ = (best + 1) % lanes;
        return best;
    }
    // gives a lease back (every exit of a call, the failed ones included); a lane nobody leased stays at 0
    void give(int lane)
    {
        if (lane >= 0 && lane < kMaxLanes && leased_[lane] > 0) leased_[lane] -= 1;
    }
    int leased(int lane) const { return lane >= 0 && lane < kMaxLanes ? leased_[lane] : 0; }
    // calls that hold a lease on any lane
    int total() const
    {
        int n = 0;
        for (int i = 0; i < kMaxLanes; ++i) n += leased_[i];
        return n;
    }

private:
    int leased_[kMaxLanes] = {};
    int next_ = 0;
};

} // namespace sqy
