// dmx_sweep.hpp -- the order in which integrate_free's workgroups walk the slab's tiles.
//
// Host and device, no HIP needed: the mapping is tested on the CPU (tests/test_sweep_order.py).
// A contact-free tick reads the very lines the tick before it read and wrote, and an XCD's 4 MiB L2 keeps its contents
// from one launch to the next; but a sweep over more bytes than the cache holds, walked in the same order every time, has
// evicted every line by the time it returns to it.  So alternate launches walk the tiles in opposite directions: the lines
// a launch touched last are the ones the next launch touches first.
//   rev == 0   block b works on tile group b
//   rev == 1   block b works on tile group (G8/8 - 1 - b/8)*8 + b%8: the groups of eight in reverse, each group in place
// b % 8 is kept on purpose.  Workgroups are observed to be dealt round-robin over the 8 XCDs (b and b + 8 share one), so a tile
// group stays with the same XCD -- the same L2 -- in both directions; a plain G - 1 - b would send it to the XCD of 7 - b%8.
// That placement is an observed property relied on for SPEED ONLY.  Correctness rests on one thing: for every grid size
// G8 that is a multiple of 8 the mapping is a bijection on [0, G8), whatever workgroup runs where and when.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DMX_SWEEP_FN __host__ __device__ __forceinline__
#else
#define DMX_SWEEP_FN inline
#endif

namespace dmx {

constexpr unsigned kSweepGroup = 8;      // XCDs of the chip = workgroups per round of the dispatcher's dealing

// the grid size the mapping is defined on: `blocks` rounded up to a whole number of groups
DMX_SWEEP_FN unsigned sweep_grid(unsigned blocks) { return (blocks + (kSweepGroup - 1)) / kSweepGroup * kSweepGroup; }

// b in [0, G8), G8 % 8 == 0, rev in {0, 1}
DMX_SWEEP_FN unsigned sweep_block(unsigned b, unsigned G8, int rev)
{
    if (rev == 0) return b;
    return (G8 / kSweepGroup - 1 - b / kSweepGroup) * kSweepGroup + b % kSweepGroup;
}

}  // namespace dmx
