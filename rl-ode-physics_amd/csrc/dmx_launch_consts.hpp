// dmx_launch_consts.hpp -- what the general tick computes from the launch's constants alone, computed once per launch.
//
// Host side only, no HIP: the rule is tested on the CPU (tests/test_launch_consts.py).  With mass and inertia as kernel arguments
// (StepParams::uni, OPT_UNI in dmx_kernels.hip) the general tick (dmx_step_fused.hpp: tick_head / tick_tail; dmx_math.hpp:
// add_gyro_torque) divides by values that every lane of every wavefront of the launch holds alike:
//   1 / Ib.k    (tick_head: the body-frame inverse inertia)
//   1 / m       (the callers' invMass, which enters the tick as hm = h * (1 / m))
//   1 / h       (add_gyro_torque, the implicit form)
// and asks whether Ib is isotropic.  The compiler hoists all of that out of the grid-stride loop -- it is loop-invariant and
// cannot trap -- so each wavefront ran five IEEE divisions and their kin ahead of its first load, for values that a launch that
// takes the short tick (dmx_torque_free.hpp) does not even use.  launch_consts computes them here with the tick's own operations,
// in the batch's precision; they travel as scalar kernel arguments of their own beside `tf` (whose hm = h * (1 / m) and
// mg.k = fma(m, g.k, 0) are the two products of constants the tick needs; TorqueFree and torque_free_plan stay as they are), and
// the tick (dmx_step_fused.hpp: tick_head_with, fed by TickGiven) reads them where the dividing form (TickDivides) divides.
// StepParams does not grow.
// The constants are used iff m, every Ib.k and h are finite and not zero and every reciprocal is finite.  Anything else -- a zero,
// an infinity, a NaN, a denormal whose reciprocal overflows -- and the launch drops OPT_UNI: it takes the instantiation that
// loads mass and inertia per lane and divides per lane, as a batch with mixed constants does.  What a division by zero, an
// infinity or a NaN's payload comes to therefore never depends on the host's arithmetic agreeing with the device's; for finite
// non-zero operands with a finite quotient both are the correctly rounded IEEE quotient (denormal results included: the library's
// kernels run with denormals on).
#pragma once
#include <stdint.h>

namespace dmx {

template <class T> struct LaunchConsts {     // kernel arguments of integrate_free
    int on = 0;                              // 0: not to be used (the launch must not take an OPT_UNI instantiation)
    int iso = 0;                             // Ib.x == Ib.y && Ib.y == Ib.z (dmx_math.hpp: isotropic)
    T inv_Ib[3] = { T(0), T(0), T(0) };      // T(1) / Ib.k
    T inv_m = T(0);                          // T(1) / m; the tick's hm = h * inv_m is tf.hm
    T inv_h = T(0);                          // T(1) / h
};

inline bool lc_finite(float x)  { return x - x == 0.0f; }      // false for +-inf and NaN
inline bool lc_finite(double x) { return x - x == 0.0; }

template <class T>
inline LaunchConsts<T> launch_consts(T mass, const T Ib[3], T h)
{
    LaunchConsts<T> lc;
    bool on = true;
    const T in[5] = { Ib[0], Ib[1], Ib[2], mass, h };
    T inv[5];
    for (int k = 0; k < 5; k++) {
        inv[k] = T(1) / in[k];
        on = on && lc_finite(in[k]) && in[k] != T(0) && lc_finite(inv[k]);
    }
    for (int k = 0; k < 3; k++) lc.inv_Ib[k] = inv[k];
    lc.inv_m = inv[3];
    lc.inv_h = inv[4];
    lc.iso = (Ib[0] == Ib[1] && Ib[1] == Ib[2]) ? 1 : 0;
    lc.on = on ? 1 : 0;
    return lc;
}

}  // namespace dmx
