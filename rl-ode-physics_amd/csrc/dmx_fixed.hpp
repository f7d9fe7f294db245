// dmx_fixed.hpp -- may this contact-free launch leave out the loads of state a tile has proven fixed?
//
// Host side only, no HIP: the rule is tested on the CPU (tests/test_fixed_chain.py).  integrate_free keeps one word per
// 64-body tile on the device: bit k says that a launch loaded pos.k and lvel.k of the tile's active lanes, ran the tick and found
// both components' bits unchanged in every lane.  free_body_step computes the new lvel.k and pos.k from the old lvel.k and pos.k,
// h, g.k, the mass and the force accumulator (zero outside the EXT kernel) alone, so the same inputs give the same bits again,
// tick after tick -- until one of those inputs changes or somebody else writes the slab.  The words therefore stand only along an
// unbroken CHAIN of launches, and this record is the chain: it is told about every event and answers, before each contact-free
// launch, which of three things the launch is.
//   FIX_OFF        the launch knows nothing of the words (and breaks the chain: it steps bodies behind their back)
//   FIX_ESTABLISH  loads everything, as ever, and writes every tile's word with what it observed
//   FIX_LEAN       reads the tile's word first and, for a fixed lateral axis, issues neither the two loads nor the ballots and stores
// A launch may ESTABLISH if it is an eligible instantiation (one tick, no force accumulators, store elision on) over the whole
// active slab, with no skip mask and no gate.  It is LEAN if, besides, the launch before it onto these slots was an establishing
// or lean one with the same key (h and g in the kernel's precision, mass source and value, gyro mode, n_active, elision mask),
// nothing has happened in between, and it runs in place with no safe-zone check and no boundary pack (those read pos.x / pos.z).
// Doors that break the chain (brk): every entry point of the C ABI other than the stepping calls themselves and dmxBatchDownload,
// which only reads the slab and closes the open chunk without touching the record (dmx_settle does both for the others), every
// writer of state (dmx_state_written), snapshot restore and rollback, the exact tick, the joints tick, and any launch that is
// not establish or lean.  Two events end it for good (end): a device pointer into the slab, and a stepping call made while the
// stream is being captured -- replays of a graph run behind the library's back.
// The record is conservative: it may say establish or off where lean would have been right, never lean where it is not.
#pragma once
#include <stdint.h>
#include <string.h>

namespace dmx {

enum : int { FIX_OFF = 0, FIX_ESTABLISH = 1, FIX_LEAN = 2 };

struct FixedKey {          // what a fixed axis's bits depend on besides the slab: equal keys, equal ticks
    uint64_t h = 0, g[3] = { 0, 0, 0 }, mass = 0;      // bit patterns, in the kernel's precision
    int mass_uniform = 0;                              // the mass is a kernel argument (its value is `mass`), not the slab's
    int gyro = 0, elide = 0;
    int64_t n_active = 0;
    bool operator==(const FixedKey &o) const
    {
        return h == o.h && g[0] == o.g[0] && g[1] == o.g[1] && g[2] == o.g[2] && mass_uniform == o.mass_uniform &&
               (!mass_uniform || mass == o.mass) && gyro == o.gyro && elide == o.elide && n_active == o.n_active;
    }
    template <class T> static uint64_t bits(T v) { uint64_t u = 0; memcpy(&u, &v, sizeof(T)); return u; }
};

struct FixedLaunch {       // one launch that launch_step would take to integrate_free
    bool eligible = false;         // one tick, no EXT, store elision on: an instantiation with the mode built in
    bool whole = false;            // first == 0 and count == n_active, no skip mask, no gate
    bool in_place = false, bp_check = false, pack = false;
    FixedKey key;
};

struct FixedChain {
    bool on = true;                // the switch (DMX_ELIDE_LOADS, dmxBatchSetLoadElision)
    bool ended = false;            // for good
    bool live = false;             // the words describe the current slab under `key`
    FixedKey key;
    int64_t n_establish = 0, n_lean = 0, n_breaks = 0;

    void brk() { if (live) { live = false; n_breaks++; } }
    void end() { brk(); ended = true; }
    void set_on(bool v) { brk(); on = v; }

    // the launch about to be enqueued; the answer goes into it
    int next(const FixedLaunch &L)
    {
        if (!on || ended || !L.eligible || !L.whole) { brk(); return FIX_OFF; }
        if (live && L.key == key && L.in_place && !L.bp_check && !L.pack) { n_lean++; return FIX_LEAN; }
        if (live && !(L.key == key)) n_breaks++;
        live = true; key = L.key;
        n_establish++;
        return FIX_ESTABLISH;
    }
};

}  // namespace dmx
