// C entry points around dmx::sweep_block / dmx::sweep_grid (csrc/dmx_sweep.hpp) for tests/test_sweep_order.py: plain g++, no HIP.
#include "dmx_sweep.hpp"

// out[b] = sweep_block(b, G8, rev) for b in [0, G8)
extern "C" void sweep_table(unsigned G8, int rev, unsigned *out)
{
    for (unsigned b = 0; b < G8; b++) out[b] = dmx::sweep_block(b, G8, rev);
}

extern "C" unsigned sweep_grid_of(unsigned blocks) { return dmx::sweep_grid(blocks); }
