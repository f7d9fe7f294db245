// dmx_lean_tick.hpp -- the tick of a body in a tile whose lateral axes (x, z) are proven fixed, and the arguments of the kernel
// that runs it (dmx_kernels.hip: integrate_free_lean).
//
// Host and device: the tick is tested on the CPU (tests/test_lean_tick.py).  A lean launch (dmx_fixed.hpp) of a scene under
// gravity along y loads neither pos.x / pos.z nor lvel.x / lvel.z of a tile whose word says they stay as they are; with the
// short tick of a body without torque (dmx_torque_free.hpp) what is left of tick_integrate is
//   v.y = fma(hm, mg.y, v.y) ; w.k += +0 ; x.y = fma(h, v.y, x.y) ; integrate_quat(q, w, h)
// -- torque_free_step without the two fmas per lateral axis, whose results such a tile neither tests nor stores.  Composed from
// the pieces tick_integrate itself is made of (dmx_math.hpp), not restated: the same operations on the same values, same bits.
#pragma once
#include <stdint.h>
#include "dmx_math.hpp"

namespace dmx {

// (w + (+0) turns -0 into +0 and quiets a signalling NaN: the add stays, as in torque_free_step)
template <class T> DMX_HD void lean_tick(T &xy, Q4<T> &q, T &vy, V3<T> &w, T hm, T mgy, T h)
{
    tick_kick_axis(vy, hm, mgy);
    tick_turn(w, V3<T>{ T(0), T(0), T(0) });
    tick_drift_axis(xy, h, vy);
    integrate_quat(q, w, h);
}

// What a wavefront of integrate_free_lean on its straight line reads, in one aligned run at the head of the kernel's arguments;
// whatever the shared tile body needs for any other wavefront (StepParams and the launch's constants) travels behind it.
// g8: the grid's size in workgroups, a multiple of 8 (dmx_sweep.hpp) -- the kernel does not ask the dispatch packet for it.
// The first 32 bytes are what stands between a wavefront and its loads (one scalar load of eight dwords); the tick's three reals follow.
template <class T> struct alignas(32) LeanHot {
    int64_t n;
    uint32_t g8;
    int32_t rev;
    T *S;
    uint32_t *fix_words;
    T h, hm, mgy;
};

}  // namespace dmx
