// C entry points around csrc/dmx_fixed.hpp for tests/test_fixed_chain.py: the record alone, no HIP.
#include <stdint.h>
#include "dmx_fixed.hpp"

using dmx::FixedChain;
using dmx::FixedLaunch;

extern "C" {

void *fc_new(void) { return new FixedChain(); }
void fc_free(void *p) { delete (FixedChain *)p; }
void fc_brk(void *p) { ((FixedChain *)p)->brk(); }
void fc_end(void *p) { ((FixedChain *)p)->end(); }
void fc_set_on(void *p, int on) { ((FixedChain *)p)->set_on(on != 0); }

// flags: bit 0 eligible, 1 whole, 2 in place, 3 bp_check, 4 pack, 5 mass is a kernel argument
// key: h, g.x, g.y, g.z, mass as bit patterns, then gyro, elide, n_active
int fc_next(void *p, int flags, const uint64_t key[8])
{
    FixedLaunch L;
    L.eligible = (flags & 1) != 0; L.whole = (flags & 2) != 0; L.in_place = (flags & 4) != 0;
    L.bp_check = (flags & 8) != 0; L.pack = (flags & 16) != 0;
    L.key.mass_uniform = (flags & 32) ? 1 : 0;
    L.key.h = key[0]; L.key.g[0] = key[1]; L.key.g[1] = key[2]; L.key.g[2] = key[3]; L.key.mass = key[4];
    L.key.gyro = (int)key[5]; L.key.elide = (int)key[6]; L.key.n_active = (int64_t)key[7];
    return ((FixedChain *)p)->next(L);
}

// establish launches, lean launches, breaks, ended
void fc_stats(void *p, int64_t out[4])
{
    const FixedChain *c = (const FixedChain *)p;
    out[0] = c->n_establish; out[1] = c->n_lean; out[2] = c->n_breaks; out[3] = c->ended ? 1 : 0;
}

}
