// dmx_amotor.hpp -- the angular motor's own geometry (include/dmx_batch.h at DMX_JOINT_AMOTOR): three coupled axes and three angles
// from two body poses.  It runs in a kernel of its own in front of the tick (amotor_prepare, dmx_artic.hip), never inside an island
// kernel: those have no registers to spare for three atan2 and a normalisation (dmx_island_rows.hpp at half_angle_atan2), and read
// the prepared reals of an axis instead (amotor_unit_row).  The limit / motor table of every axis is worked out here too: with
// limot_table called from amotor_unit_row five island kernels gained scratch (profiles/amotor_kernel_resources.txt), so c, lo and hi
// travel in the prepared table beside the axis and its angle.
// (host too: the ODE face's dJointGetAMotorAngle / AngleRate, tests/harness/amotor_rows_harness.cpp)
#pragma once
#include <math.h>
#include "../../include/dmx_batch.h"
#include "dmx_math.hpp"
#include "dmx_island_rows.hpp"      // limot_table

namespace dmx {

// (the prepared table's layout, AMOTOR_PREP_REALS / AMOTOR_AXIS_REALS / AMP_*: dmx_internal.hpp, beside the unit's marker)
// what amotor_prepare reads per joint of the set, staged by the host with the tick's other tables: active = the joint is an AMotor
// that is active this tick (the host knows the flags); body1 / body2 = its sides AS GIVEN (-1: the world)
struct AMotorIn { int32_t active, body1, body2, pad; dmxAMotor m; };
// one lane per joint of the set: prep[24 j ..] (zeros for a joint that is not an active AMotor), k = ERP / h as the island kernels
// form it, and, when rates is not null, rates[3 j + i] = a_i . (omega_1 - omega_2)
template <class T>
hipError_t launch_amotor_prepare(const T *S, int64_t stride, const AMotorIn *in, int nj, T k, T *prep, T *rates, hipStream_t st);

template <class T> DMX_HD T amotor_atan2(T y, T x);
template <> DMX_HD float amotor_atan2<float>(float y, float x) { return ::atan2f(y, x); }
template <> DMX_HD double amotor_atan2<double>(double y, double x) { return ::atan2(y, x); }

// a[0..3), th[0..3) of an AMotor in the sides AS GIVEN: has_i = side i is a body with quaternion q_i (a world side: R = 1).  Axes and
// angles of unused axes (i >= num_axes) are zero.
template <class T>
DMX_HD void amotor_axes(bool has1, const Q4<T> &q1, bool has2, const Q4<T> &q2, const dmxAMotor &m, V3<T> *a, T *th)
{
    const V3<T> zero = { T(0), T(0), T(0) };
    M3<T> R1, R2;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R1.m[i][j] = R2.m[i][j] = i == j ? T(1) : T(0);
    if (has1) R1 = quat_to_R(q1);
    if (has2) R2 = quat_to_R(q2);
    auto vec = [](const double *p) -> V3<T> { return { (T)p[0], (T)p[1], (T)p[2] }; };
    for (int i = 0; i < 3; i++) { a[i] = zero; th[i] = T(0); }
    if (m.mode == DMX_AMOTOR_EULER) {
        a[0] = mulv(R1, vec(m.axis[0]));
        a[2] = mulv(R2, vec(m.axis[2]));
        const V3<T> c = cross(a[2], a[0]);
        const T len = tsqrt<T>(dot(c, c));
        if (len > T(0)) a[1] = { c.x / len, c.y / len, c.z / len };
        const V3<T> r1 = mulv(R1, vec(m.ref1)), r2 = mulv(R2, vec(m.ref2));
        th[0] = -amotor_atan2<T>(dot(a[2], cross(a[0], r1)), dot(a[2], r1));
        th[1] = -amotor_atan2<T>(dot(a[2], a[0]), dot(a[2], cross(a[0], a[1])));
        th[2] = -amotor_atan2<T>(dot(r2, a[1]), dot(r2, cross(a[1], a[2])));
        return;
    }
    for (int i = 0; i < 3; i++) {
        if (i >= m.num_axes) break;
        const V3<T> ax = vec(m.axis[i]);
        a[i] = m.rel[i] == 1 ? mulv(R1, ax) : m.rel[i] == 2 ? mulv(R2, ax) : ax;
        th[i] = (T)m.angle[i];
    }
}

// one joint's entry of the prepared table (amotor_prepare's lane; host too: tests/harness/amotor_rows_harness.cpp): the axes and
// angles, and per axis c, lo, hi from the table with x = theta_i, the axis's stops, vel and fmax in the batch's precision, k = ERP / h
template <class T>
DMX_HD void amotor_prepare_joint(bool has1, const Q4<T> &q1, bool has2, const Q4<T> &q2, const dmxAMotor &m, T k, T *out, V3<T> *a)
{
    T th[3];
    amotor_axes<T>(has1, q1, has2, q2, m, a, th);
    for (int i = 0; i < 3; i++) {
        T *o = out + AMOTOR_AXIS_REALS * i;
        o[AMP_AXIS] = a[i].x; o[AMP_AXIS + 1] = a[i].y; o[AMP_AXIS + 2] = a[i].z; o[AMP_THETA] = th[i];
        T c, lo, hi;
        limot_table(th[i], (T)m.lo_stop[i], (T)m.hi_stop[i], (T)m.vel[i], (T)m.fmax[i], k, c, lo, hi);
        o[AMP_C] = c; o[AMP_LO] = lo; o[AMP_HI] = hi; o[AMOTOR_AXIS_REALS - 1] = T(0);
    }
}

}  // namespace dmx
