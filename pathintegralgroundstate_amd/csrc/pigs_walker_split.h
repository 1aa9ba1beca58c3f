// pigs_walker_split.h -- the walker list of one accumulator launch, and the rule that cuts a request into launches.
// Host logic only (no HIP): tests/shim/walker_split_check.cpp compiles it for the CPU.
#pragma once

#include <stdint.h>

#include <vector>

namespace pigs {

// The list goes by value in the kernel arguments (no upload, no host buffer to keep alive): a launch is queued on the
// context's stream and there is nothing to wait for.
constexpr int kWalkerListMax = 256;
struct WalkerList { int32_t w[kWalkerListMax]; };

// per walker the last launch that listed it; launch ids count up over all accumulator families of a context
struct WalkerMarks {
    std::vector<int64_t> last;
    int64_t launch = 0;
};

// The walkers of the launch that starts at sw[i0]: copied to L, their number returned.  A launch ends where the list
// does, where `cap` walkers are taken (the list or the family's scratch is full), or -- with `unique`, for the kernels
// in which one thread or workgroup owns an accumulator element per launch -- where a walker would appear in it a
// second time; the stream orders the launches, so a walker listed twice is added twice, in list order.  Without
// `unique` (integer atomics) a walker may repeat inside a launch.  A list left out by the caller (`listed` false:
// sw is 0..n-1) holds no repeats and needs no marks; with marks, marks.last holds one entry per walker.
inline int take_walkers(const std::vector<int32_t> &sw, bool listed, int i0, int cap, bool unique, WalkerMarks &marks,
                        WalkerList &L)
{
    const int n = (int)sw.size();
    const bool check = unique && listed;
    const int64_t launch = ++marks.launch;
    int m = 0;
    while (i0 + m < n && m < cap && !(check && marks.last[sw[i0 + m]] == launch)) {
        if (check) marks.last[sw[i0 + m]] = launch;
        L.w[m] = sw[i0 + m];
        ++m;
    }
    return m;
}

} // namespace pigs
