// dmx_small.hpp -- the single-launch tick of small worlds (dmx_small.hip): what dmxBatchStepJoints does for a world of a few
// hundred bodies at most in ONE kernel launch, its tables read from host-mapped pinned staging and the new body state written
// to the slab and to a host-mapped mirror ("Single-launch tick for small worlds").
#pragma once

#include "dmx_batch_priv.hpp"
#include "dmx_autodisable.hpp"

namespace dmx {

// eligibility caps: the reference never holds more than MAX_BODIES = 512 bodies (inc/body.h:6), and every body may be an island
// of its own.  QuickStep: one-body islands of up to eight contacts are the tail's, a lane each, so the grid is at most 256
// workgroups of islands with two bodies or more plus 512 / SMALL_TAIL_LANES = 64 of the tail (more only if bodies carry nine
// contacts or more); dWorldStep: every island with rows is a workgroup, 512 at most, plus two of the tail.  A few hundred
// workgroups on the chip's 256 compute units either way.
constexpr int SMALL_MAX_BODIES = 512;
constexpr int SMALL_MAX_ISLANDS = 512;
// islands a workgroup of the kernel's tail steps one lane each (QuickStep: free bodies and one-body islands of 1..8 contacts;
// eight lanes keep solve_singles_lds_body's rows at 18 KB of LDS in f64); dWorldStep's tail holds free bodies only, a lane each
constexpr int SMALL_TAIL_LANES = 8;

template <class T> struct SmallTick {
    T *mirror;             // host-mapped: 13 reals per slot, DMX_STATE order
    StepDiag *diag_next;   // the diagnostics slot the NEXT small tick accumulates into: zeroed here
    int n_slots;           // the batch's capacity
    int full;              // 1: the mirror was not valid before this tick -- the slots no island steps are copied too
    int lds_bodies;        // QuickStep: accumulators of up to this many island bodies in LDS (as launch_islands chooses)
    int murty; T tol_rel;  // dWorldStep: lcp_island_lds' pivoting mode and tolerance (as launch_lcp_lds chooses)
    // auto-disable, read by the kernel's AD instantiation only: the device's flag bytes as the view idle_update reads and writes, the
    // host-mapped flag mirror (one byte per slot, filled by the host before the launch: SMALL_AD_SKIPPED marks the slots of asleep
    // islands), the per-slot counters and the rule's parameters
    uint8_t *ad_flags = nullptr, *ad_mirror = nullptr;
    int32_t *ad_steps = nullptr; double *ad_time = nullptr;
    IdleParams<T> ad;
};
// in the host-mapped flag mirror only, never in a flag byte: the tick left this live slot out (an asleep island)
constexpr uint8_t SMALL_AD_SKIPPED = 0x80;

template <class T>
hipError_t launch_small_tick(T *S, const uint8_t *bflags, int64_t stride, const IslandSet<T> &I, const StepParams<T> &P, StepDiag *diag,
                             const SmallTick<T> &K, const FeedbackSet<T> &F, bool exact, size_t lds_bytes, hipStream_t st, bool pyramid = false, bool ad = false);      // (F.mode: the kernel's FB instantiation; pyramid: its APX one, QuickStep only; ad: its AD one)
// dynamic LDS of the QuickStep form for islands of up to max_bodies bodies (out: SmallTick::lds_bodies)
size_t small_tick_sor_lds(int real_bytes, int max_bodies, int *lds_bodies);
hipError_t dmx_touch_small(int real_bytes);

}  // namespace dmx
