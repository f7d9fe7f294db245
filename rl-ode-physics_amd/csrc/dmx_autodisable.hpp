// dmx_autodisable.hpp -- auto-disable (include/dmx_batch.h, "auto-disable"): the end-of-tick rule of one body, for the host and
// the device.  Two callers: autodisable_update (dmx_autodisable.hip) behind the general path's kernels, and small_world_tick's AD
// instantiation (dmx_small.hip) where a thread has finished a body.  tests/harness/autodisable_harness.cpp runs it on the host.
#pragma once

#include "dmx_internal.hpp"

namespace dmx {

enum : int { BF_AUTODISABLE = 16, BF_DISABLED = 32 };

// lin2 / ang2: the thresholds squared, in the batch's precision, as the speeds they are compared with; the time is a double in
// both precisions, so that a run of subtractions of h ends on the same tick in f32 and f64
template <class T> struct IdleParams {
    T lin2, ang2;
    int idle_steps;
    double idle_time, h;
};
template <class T> inline IdleParams<T> make_idle_params(double lin, double ang, int idle_steps, double idle_time, double h)
{
    IdleParams<T> A;
    A.lin2 = (T)lin * (T)lin; A.ang2 = (T)ang * (T)ang;
    A.idle_steps = idle_steps; A.idle_time = idle_time; A.h = h;
    return A;
}

// Slot s has been stepped by this tick: count it idle or reset its counters, and put it to sleep when both have run out.
// `flags` is the one view of the flag bytes this function reads and writes; a caller that holds a const view of the same bytes
// must be done reading slot s's byte through it.  Returns the slot's byte as it stands afterwards.
template <class T>
DMX_HD uint8_t idle_update(T *S, uint8_t *flags, int32_t *steps_left, double *time_left, const IdleParams<T> &A, int s)
{
    const uint8_t f = flags[s];
    if ((f & (BF_ALIVE | BF_AUTODISABLE | BF_KINEMATIC | BF_DISABLED)) != (BF_ALIVE | BF_AUTODISABLE)) return f;
    const T lx = S[slab_ix(C_LVEL + 0, s)], ly = S[slab_ix(C_LVEL + 1, s)], lz = S[slab_ix(C_LVEL + 2, s)];
    const T ax = S[slab_ix(C_AVEL + 0, s)], ay = S[slab_ix(C_AVEL + 1, s)], az = S[slab_ix(C_AVEL + 2, s)];
    const bool idle = (lx * lx + ly * ly + lz * lz <= A.lin2) && (ax * ax + ay * ay + az * az <= A.ang2);
    int32_t st = A.idle_steps;
    double tl = A.idle_time;
    if (idle) {
        st = steps_left[s] - 1; if (st < 0) st = 0;
        tl = time_left[s] - A.h; if (tl < 0.0) tl = 0.0;
    }
    steps_left[s] = st;
    time_left[s] = tl;
    if (st != 0 || tl != 0.0) return f;
    const uint8_t g = (uint8_t)(f | BF_DISABLED);
    flags[s] = g;
#pragma unroll
    for (int c = 0; c < 6; c++) S[slab_ix(C_LVEL + c, s)] = T(0);
    return g;
}

// the general path's kernel: one lane per stepped slot (dmx_autodisable.hip)
template <class T>
hipError_t launch_autodisable_update(T *S, uint8_t *flags, int32_t *steps_left, double *time_left, const IdleParams<T> &A, const int *bodies, int n_bodies,
                                     int n_slots, hipStream_t st);

}  // namespace dmx
