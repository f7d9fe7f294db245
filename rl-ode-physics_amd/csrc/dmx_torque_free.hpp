// dmx_torque_free.hpp -- may this contact-free launch take the short tick of a body without torque?
//
// Host side only, no HIP: the rule is tested on the CPU (tests/test_torque_free.py).  A body without rows whose torque
// accumulator is exactly (+0, +0, +0) -- no force accumulators in the launch, no gyroscopic torque -- gets from the general tick
// (dmx_step_fused.hpp: tick_head / tick_tail)
//   w += R diag(1/Ib) R^T (h * (+0, +0, +0))
// which is w + (+0) per component whenever the rotated inverse inertia is finite: its diagonal entries are sums of
// R_ij (d_j R_ij) >= +0, so every component of the product is a chain of three signed zeros of which one is +0, hence +0.  The
// short tick (dmx_math.hpp: torque_free_step) adds that +0 and builds neither R nor the inverse inertia; the kernel takes it for
// a wavefront whose every active lane has |q.k| <= 2 (torque_free_admits: R finite, entries <= 17) when this rule says "on".
// The path is on iff
//   - the switch is on (DMX_TORQUE_FREE, dmxBatchSetTorqueFree);
//   - mass and inertia travel as kernel arguments (StepParams::uni; hence never under graph capture);
//   - the launch has no force accumulators;
//   - gyro == 0, or the inertia is isotropic (dmx_math.hpp: isotropic -- the general tick's own early-out);
//   - h is finite and > 0;
//   - every Ib.k > 0 with 1/Ib.k finite and at most max_finite / 1024: with entries of R <= 17 and 3 * 17^2 < 1024 the rotated
//     inverse inertia stays finite.  A zero or denormal inertia, whose inverse is inf, switches the path off; so does a NaN.
// The rule also computes, once per launch, what the general tick computes per lane per tick from the same constants with the
// same operations: hm = h * (1 / m) and mg.k = fma(m, g.k, 0).  They travel as scalar kernel arguments of their own beside
// `rev` and `fix_mode`; StepParams does not grow.
#pragma once
#include <stdint.h>

namespace dmx {

template <class T> struct TorqueFree {       // kernel arguments of integrate_free
    int on = 0;
    T hm = T(0), mg[3] = { T(0), T(0), T(0) };
};

inline float  tf_fma(float a, float b, float c)    { return __builtin_fmaf(a, b, c); }
inline double tf_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
inline float  tf_max_finite(float)  { return __FLT_MAX__; }
inline double tf_max_finite(double) { return __DBL_MAX__; }

// uni: the constants are kernel arguments, and mass / Ib are their values in the batch's precision; ext: force accumulators are set
template <class T>
inline TorqueFree<T> torque_free_plan(bool enabled, bool uni, bool ext, int gyro, T mass, const T Ib[3], T h, const T g[3])
{
    TorqueFree<T> tf;
    tf.hm = h * (T(1) / mass);
    for (int k = 0; k < 3; k++) tf.mg[k] = tf_fma(mass, g[k], T(0));
    bool on = enabled && uni && !ext;
    on = on && (gyro == 0 || (Ib[0] == Ib[1] && Ib[1] == Ib[2]));
    on = on && h > T(0) && h <= tf_max_finite(h);
    for (int k = 0; k < 3; k++) {
        const T inv = T(1) / Ib[k];
        on = on && Ib[k] > T(0) && inv <= tf_max_finite(inv) / T(1024);
    }
    tf.on = on ? 1 : 0;
    return tf;
}

}  // namespace dmx
