// dmx_damping.hpp -- velocity damping and the angular speed cap (include/dmx_batch.h, "damping"): the start-of-tick rule of one
// body and the integrator's cap, for the host and the device.  Callers: damping_apply (dmx_damping.hip) in front of a
// dmxBatchStepJoints tick's first kernel, on the general path and in front of the single-launch tick alike, and finish_body
// (dmx_island_rows.hpp) for the cap.  tests/harness/damping_harness.cpp runs both on the host.
#pragma once

#include "dmx_internal.hpp"

namespace dmx {

// the per-slot table on the device: DAMP_REALS reals per slot in the batch's precision, dmxBodyDamping's fields in their order
enum : int { DAMP_LIN_SCALE = 0, DAMP_ANG_SCALE = 1, DAMP_LIN_THRESHOLD = 2, DAMP_ANG_THRESHOLD = 3, DAMP_MAX_ANG_SPEED = 4, DAMP_REALS = 5 };

// Slot s is about to be stepped: scale its pre-tick velocities.  threshold^2 and 1 - scale are formed in the batch's precision;
// the comparison is strict.  A slot that is not ALIVE, or is KINEMATIC, keeps its bits.
template <class T>
DMX_HD void damp_body(T *S, const uint8_t *flags, const T *table, int s)
{
    if ((flags[s] & (BF_ALIVE | BF_KINEMATIC)) != BF_ALIVE) return;
    const T *d = table + (size_t)DAMP_REALS * (size_t)s;
    const T ls = d[DAMP_LIN_SCALE], as = d[DAMP_ANG_SCALE];
    if (ls != T(0)) {
        const T x = S[slab_ix(C_LVEL + 0, s)], y = S[slab_ix(C_LVEL + 1, s)], z = S[slab_ix(C_LVEL + 2, s)];
        const T t = d[DAMP_LIN_THRESHOLD];
        if (x * x + y * y + z * z > t * t) {
            const T k = T(1) - ls;
            S[slab_ix(C_LVEL + 0, s)] = x * k; S[slab_ix(C_LVEL + 1, s)] = y * k; S[slab_ix(C_LVEL + 2, s)] = z * k;
        }
    }
    if (as != T(0)) {
        const T x = S[slab_ix(C_AVEL + 0, s)], y = S[slab_ix(C_AVEL + 1, s)], z = S[slab_ix(C_AVEL + 2, s)];
        const T t = d[DAMP_ANG_THRESHOLD];
        if (x * x + y * y + z * z > t * t) {
            const T k = T(1) - as;
            S[slab_ix(C_AVEL + 0, s)] = x * k; S[slab_ix(C_AVEL + 1, s)] = y * k; S[slab_ix(C_AVEL + 2, s)] = z * k;
        }
    }
}

// the integrator's cap: |w| > max  ->  w *= max / |w|.  With max = +inf the test is never true (inf * inf = inf).
template <class T>
DMX_HD void cap_angular_speed(V3<T> &w, T max_speed)
{
    const T ww = w.x * w.x + w.y * w.y + w.z * w.z;
    if (ww > max_speed * max_speed) {
        const T k = max_speed / tsqrt<T>(ww);
        w.x *= k; w.y *= k; w.z *= k;
    }
}

// the kernel: one lane per stepped slot over the tick's body list (dmx_damping.hip)
template <class T>
hipError_t launch_damping(T *S, const uint8_t *flags, const T *table, const int *bodies, int n_bodies, int n_slots, hipStream_t st);

}  // namespace dmx
