// dmx_island_rows.hpp -- the per-body / per-contact / per-row phase functions of the general island step (gravity and
// world-frame inertia, the rows of a contact joint and of the units of a ball, hinge, slider or fixed joint, rhs and M^-1 J^T, one SOR row update, the integration of a body).
// Shared by the SOR kernels (dmx_islands.hip) and the exact solve of dWorldStep (dmx_lcp.hip): both steppers build the same
// rows [ODE-recall: dxStepIsland / dxQuickStepIsland share getInfo1/getInfo2], /root/reference/src/main.c:213.
#pragma once
#include <hip/hip_runtime.h>
#include "dmx_internal.hpp"
#include "dmx_math.hpp"
#include "dmx_damping.hpp"

namespace dmx {

// per-row scratch layout (reals)
// (29 fields in ISLAND_ROW_REALS = 32 reals: a row is one aligned 128-byte line in f32 (two in f64) and solve_island_wg fetches it as
//  16-byte pieces -- eight requests that touch one line instead of 29 that touch two: a large island's sweeps are bound by how many
//  cache-line look-ups its lanes' scattered rows cost the compute unit's one L1, see row_load)
enum : int { RW_J = 0, RW_IMJ = 12, RW_RHS = 24, RW_AD = 25, RW_LO = 26, RW_HI = 27, RW_LAM = 28, RW_COUNT = ISLAND_ROW_REALS };
// the first of the three spare reals: in a tick made with feedback on (the FB instantiations) QuickStep's row_setup leaves the factor Ad it scaled J by here
enum : int { RW_UNSCALE = 29 };
// the other two, in a tick with pyramid rows or extended surfaces (DMX_CONTACT_APPROX1, DMX_CONTACT_SURFACE_EXT; the APX instantiations,
// which alone write and read them): RW_FMU = the row's mu on a pyramid row, -1 on the normal row of a contact that has one, 0 on every other row; RW_FDIR = the pyramid row's direction
// (1 or 2): its contact's normal row is that many rows before it
enum : int { RW_FMU = 30, RW_FDIR = 31 };
static_assert(RW_COUNT >= 29 && RW_COUNT % 4 == 0, "a row is read in 16-byte pieces");
// per island-body scratch layout (reals)
enum : int { BW_INVI = 0, BW_FACC = 9, BW_TACC = 12, BW_INVM = 15, BW_FC = 16, BW_TMP = 22, BW_COUNT = 28 };

// (host too: tests/harness/joint_rows_harness.cpp runs joint_unit_rows on the CPU)
template <class T> DMX_HD V3<T> ld3(const T *p) { return { p[0], p[1], p[2] }; }
template <class T> DMX_HD void st3(T *p, const V3<T> &v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }
template <class T> DMX_HD T dot3p(const T *a, const V3<T> &b) { return fma_(a[2], b.z, fma_(a[1], b.y, a[0] * b.x)); }
template <class T> DMX_HD V3<T> ldS(const T *S, int64_t stride, int c0, int s)
{
    return { S[slab_ix(c0 + 0, s)], S[slab_ix(c0 + 1, s)], S[slab_ix(c0 + 2, s)] };
}

// ---- stage 0, body k of the island: gravity, world-frame inverse inertia, gyroscopic torque ---------------
template <class T>
DMX_HD void stage_body(const T *S, const uint8_t *bflags, int64_t stride, const IslandSet<T> &I,
                                           const StepParams<T> &P, T *b, int s, int k)
{
    I.local[s] = k;
    const uint8_t fl = bflags[s];
    const Q4<T> q = { S[slab_ix(C_QUAT + 0, s)], S[slab_ix(C_QUAT + 1, s)],
                      S[slab_ix(C_QUAT + 2, s)], S[slab_ix(C_QUAT + 3, s)] };
    const V3<T> w = ldS(S, stride, C_AVEL, s);
    const T mass = S[slab_ix(C_MASS, s)];
    const V3<T> Ib = ldS(S, stride, C_INERTIA, s);
    V3<T> facc = ldS(S, stride, C_FORCE, s), tacc = ldS(S, stride, C_TORQUE, s);
    const bool kin = fl & BF_KINEMATIC;
    if (!kin && !(fl & BF_NOGRAVITY)) { facc.x = fma_(mass, P.g.x, facc.x); facc.y = fma_(mass, P.g.y, facc.y); facc.z = fma_(mass, P.g.z, facc.z); }
    M3<T> invIw;
    if (kin) {
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) invIw.m[i][j] = T(0);
        b[BW_INVM] = T(0);
    } else {
        const M3<T> R = quat_to_R(q);
        const V3<T> invIb = { T(1) / Ib.x, T(1) / Ib.y, T(1) / Ib.z };
        invIw = rotate_diag(R, invIb);
        if (P.gyro != 0 && !(fl & BF_NOGYRO) && !isotropic(Ib)) {
            const M3<T> Iw = rotate_diag(R, Ib);
            add_gyro_torque(tacc, Iw, w, P.h, P.gyro);
        }
        b[BW_INVM] = T(1) / mass;
    }
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) b[BW_INVI + 3 * i + j] = invIw.m[i][j];
    st3(b + BW_FACC, facc);
    st3(b + BW_TACC, tacc);
    for (int j = 0; j < 6; j++) b[BW_FC + j] = T(0);
}

// per-contact surface arrays are optional: without them every contact carries the batch's surface (StepParams)
// (an entry that is a unit of an articulation joint carries its unit's marker there, a negative number: UNIT_*_MU, and the
//  marker says how many rows the unit has)
template <class T> DMX_HD int unit_rows_of(T mu)
{
    return (mu == T(UNIT_HINGE2_MU) || mu == T(UNIT_SLIDER2_MU)) ? 2 : (mu == T(UNIT_LIMOT_MU) || mu <= T(UNIT_SLIMOT_MU)) ? 1 : 3;      // (<=: UNIT_AMOTOR_MU too)
}
template <class T> __device__ __forceinline__ int contact_rpc(const IslandSet<T> &I, const StepParams<T> &P, int ci)
{
    const T mu = I.cmu != nullptr ? I.cmu[ci] : P.mu;
    if (I.has_units && mu < 0) return unit_rows_of(mu);
    return mu > 0 ? 3 : 1;
}
template <class T> DMX_HD bool contact_is_unit(const IslandSet<T> &I, int ci)
{
    return I.has_units && I.cmu[ci] < 0;
}

// a + b and its rounding error (Knuth's TwoSum; the library is built without contraction or reassociation)
template <class T> DMX_HD T two_sum(T a, T b, T &e)
{
    const T s = a + b, bb = s - a;
    e = (a - (s - bb)) + (b - bb);
    return s;
}
// (x2 + a2) - (x1 + a1) for terms that nearly cancel
template <class T> DMX_HD T diff_of_sums(T x2, T a2, T x1, T a1)
{
    T e1, e2, e3;
    const T dx = two_sum(x2, -x1, e1), da = two_sum(a2, -a1, e2);
    const T r = two_sum(dx, da, e3);
    return r + ((e1 + e2) + e3);
}

// ---- a hinge's angle and its limit / motor row (dmxBatchSetHingeLimots; the definitions: include/dmx_batch.h) ------------------
// atan2(s, c) for c >= 0, as the half angle of a rotation needs it.  float: the library's.  double: the library's atan2 costs the
// island kernels that inline the limot row some twenty registers and with them a wave per SIMD (lcp_island_lds, lcp_prepare), so
// the double version is spelled out: with a = |s|, lo = min(a, c), hi = max(a, c) and t = lo / hi in [0, 1] the angle of (hi, lo)
// is atan(t) = 2 atan(x), x = t / (1 + sqrt(1 + t^2)) <= tan(pi/8) = 0.4142, where 24 terms of x - x^3/3 + x^5/5 - ... leave
// 0.4142^49 / 49 < 1e-20; then the reflection about pi/4 when a > c and the sign of s.  Selects, not branches, and as few of them
// as will do: in kernels that already spill scalar registers every compare costs some.
template <class T> DMX_HD T half_angle_atan2(T s, T c);
template <> DMX_HD float half_angle_atan2<float>(float s, float c) { return ::atan2f(s, c); }
template <> DMX_HD double half_angle_atan2<double>(double s, double c)
{
    const double a = s < 0.0 ? -s : s;
    const double lo = a < c ? a : c, hi = a < c ? c : a;
    const double t = lo / (hi > 0.0 ? hi : 1.0);           // (s = c = 0, no rotation at all: 0)
    const double x = t / (1.0 + __builtin_sqrt(fma_(t, t, 1.0)));
    const double y = x * x;
    double p = 1.0 / 47.0;
#pragma unroll
    for (int k = 45; k >= 1; k -= 2) p = fma_(-p, y, 1.0 / (double)k);
    double r = 2.0 * (p * x);
    r = a > c ? 1.5707963267948966 - r : r;
    return s < 0.0 ? -r : r;
}
template <class T> DMX_HD Q4<T> qconj(const Q4<T> &q) { return { q.w, -q.x, -q.y, -q.z }; }
template <class T> DMX_HD Q4<T> qmul(const Q4<T> &a, const Q4<T> &b)
{
    return { a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
             a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x, a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w };
}
// theta of the sides as given: q1, q2 = the two sides' quaternions (a world side: the identity), q0 = the stored zero pose,
// axis1 = the hinge axis in the frame of side 1.  e = conj(q1) q2 conj(q0), phi = 2 atan2(e_v . axis1, e_w) in (-pi, pi] (e and -e
// are the same rotation: the half angle is taken with e_w >= 0), theta = -phi: the angle of side 1 relative to side 2, ODE's sign.
// (host too: the ODE face's dJointGetHingeAngle, tests/harness/limot_rows_harness.cpp)
// e = conj(q1) q2 conj(q0): the rotation of side 2 against side 1 since the zero pose, in the frame of side 1
template <class T> DMX_HD Q4<T> pose_error(const Q4<T> &q1, const Q4<T> &q2, const Q4<T> &q0) { return qmul(qmul(qconj(q1), q2), qconj(q0)); }
// 2 e_v with e_w >= 0: what the angular lock of a slider or a fixed joint pulls to zero (host too: dmxBatchJointErrors' axis_err)
template <class T> DMX_HD V3<T> lock_error(const Q4<T> &e)
{
    const T two = e.w < T(0) ? T(-2) : T(2);
    return { two * e.x, two * e.y, two * e.z };
}
template <class T> DMX_HD T hinge_angle_of(const Q4<T> &e, const V3<T> &axis1)
{
    T s = fma_(e.z, axis1.z, fma_(e.y, axis1.y, e.x * axis1.x)), c = e.w;
    if (c < T(0)) { s = -s; c = -c; }
    const T pi = T(3.14159265358979323846);
    T phi = T(2) * half_angle_atan2(s, c);
    if (phi <= -pi) phi = pi;
    if (phi > pi) phi = pi;
    return -phi;
}
template <class T> DMX_HD T hinge_angle(const Q4<T> &q1, const Q4<T> &q2, const Q4<T> &q0, const V3<T> &axis1)
{
    return hinge_angle_of(pose_error(q1, q2, q0), axis1);
}

template <class T> DMX_HD Q4<T> ldq(const T *S, int s)
{
    return { S[slab_ix(C_QUAT + 0, s)], S[slab_ix(C_QUAT + 1, s)], S[slab_ix(C_QUAT + 2, s)], S[slab_ix(C_QUAT + 3, s)] };
}
// The limot unit's one row, behind its hinge's five.  The unit's reals: cpos = axis1 as given (in the frame of the given body 1,
// the world's if that side is the world), cnormal[3] + cdepth = q_0 (w, x, y, z), cbounce / cbounce_vel / csoft_erp / csoft_cfm =
// lo_stop / hi_stop / vel / fmax; cmode != 0: the sides were exchanged (given as (world, body): this entry's body 1 is the given
// body 2).  In the sides as given J = [ 0, u | 0, -u ], u = R_1 axis1: the row's velocity is theta_dot.
template <class T>
DMX_HD int limot_unit_row(const T *S, const IslandSet<T> &I, const StepParams<T> &P, T *rows, int *jb, int ci, int m, T hinv)
{
    const int s1 = I.cb1[ci], s2 = I.cb2[ci];
    const bool rev = I.cmode[ci] != 0;
    T *row = rows + (size_t)m * RW_COUNT;
    jb[2 * m] = I.local[s1]; jb[2 * m + 1] = s2 >= 0 ? I.local[s2] : -1;
    const V3<T> axis1 = ld3(I.cpos + 3 * (size_t)ci);
    // (first the angle and with it c, lo, hi, then the Jacobian: what one part needs is dead before the other begins -- the row is
    //  built inside kernels that have no registers to spare)
    {
        const Q4<T> q0 = { I.cnormal[3 * (size_t)ci + 0], I.cnormal[3 * (size_t)ci + 1], I.cnormal[3 * (size_t)ci + 2], I.cdepth[ci] };
        // the sides as given: (body 1, body 2 or the world), or after an exchange (the world, body 1)
        const int sa = rev ? -1 : s1, sb = rev ? s1 : s2;
        Q4<T> qa = { T(1), T(0), T(0), T(0) }, qb = { T(1), T(0), T(0), T(0) };
        if (sa >= 0) { qa.w = S[slab_ix(C_QUAT + 0, sa)]; qa.x = S[slab_ix(C_QUAT + 1, sa)]; qa.y = S[slab_ix(C_QUAT + 2, sa)]; qa.z = S[slab_ix(C_QUAT + 3, sa)]; }
        if (sb >= 0) { qb.w = S[slab_ix(C_QUAT + 0, sb)]; qb.x = S[slab_ix(C_QUAT + 1, sb)]; qb.y = S[slab_ix(C_QUAT + 2, sb)]; qb.z = S[slab_ix(C_QUAT + 3, sb)]; }
        const T theta = hinge_angle(qa, qb, q0, axis1);
        const T lo_s = I.cbounce[ci], hi_s = I.cbounce_vel[ci], vel = I.csoft_erp[ci], fmax = I.csoft_cfm[ci];
        const T inf = Limits<T>::inf(), k = hinv * P.erp;
        const T g = fmax > T(0) ? (vel > T(0) ? fmax : vel < T(0) ? -fmax : T(0)) : T(0);
        const bool limited = lo_s <= hi_s && (lo_s > -inf || hi_s < inf);
        T c = T(0), lo = T(0), hi = T(0);                  // inside its range, no motor: the row stays, and does nothing
        if (limited && lo_s == hi_s) { c = -k * (theta - lo_s); lo = -inf; hi = inf; }
        else if (limited && theta <= lo_s) { c = -k * (theta - lo_s); lo = g; hi = inf; }
        else if (limited && theta >= hi_s) { c = -k * (theta - hi_s); lo = -inf; hi = g; }
        else if (fmax > T(0)) { c = vel; lo = -fmax; hi = fmax; }
        row[RW_LO] = lo; row[RW_HI] = hi;
        row[RW_RHS] = c;                    // c for now
        row[RW_AD] = P.cfm;                 // cfm for now
        row[RW_LAM] = T(0);
    }
    V3<T> u = { -axis1.x, -axis1.y, -axis1.z };            // given body 1 is the world -- its axis as given -- and this entry's body 1 the given body 2
    if (!rev) {
        const Q4<T> qa = { S[slab_ix(C_QUAT + 0, s1)], S[slab_ix(C_QUAT + 1, s1)], S[slab_ix(C_QUAT + 2, s1)], S[slab_ix(C_QUAT + 3, s1)] };
        u = mulv(quat_to_R(qa), axis1);
    }
    T *J = row + RW_J;
    J[0] = J[1] = J[2] = T(0);
    st3(J + 3, u);
    for (int j = 6; j < 12; j++) J[j] = T(0);
    if (s2 >= 0) { J[9] = -u.x; J[10] = -u.y; J[11] = -u.z; }
    return 1;
}

// ---- the slider and fixed joints' units (the definitions: include/dmx_batch.h at DMX_JOINT_SLIDER) ------------------------------
// What the slider's linear unit and its limot row share, in canonical sides: a_1, a_2 (a world side: 0) and err = p_2 - p_1, formed
// as the ball unit forms it (diff_of_sums).  ci = the LINEAR unit's entry: cpos = anchor 1, cnormal = anchor 2.
template <class T>
DMX_HD void slider_arms(const T *S, int64_t stride, const IslandSet<T> &I, int ci, const M3<T> &R1, V3<T> &a1, V3<T> &a2, V3<T> &err)
{
    const int s1 = I.cb1[ci], s2 = I.cb2[ci];
    a1 = mulv(R1, ld3(I.cpos + 3 * (size_t)ci));
    const V3<T> f2 = ld3(I.cnormal + 3 * (size_t)ci);
    const V3<T> x1 = ldS(S, stride, C_POS, s1);
    V3<T> x2 = f2;
    a2 = { T(0), T(0), T(0) };
    if (s2 >= 0) { x2 = ldS(S, stride, C_POS, s2); a2 = mulv(quat_to_R(ldq(S, s2)), f2); }
    err = { diff_of_sums(x2.x, a2.x, x1.x, a1.x), diff_of_sums(x2.y, a2.y, x1.y, a1.y), diff_of_sums(x2.z, a2.z, x1.z, a1.z) };
}
// one row J = [ r, arm x r | -r, -(a2 x r) ]
template <class T> DMX_HD void slider_row_J(T *J, const V3<T> &r, const V3<T> &arm, const V3<T> &a2, bool two)
{
    st3(J, r);
    st3(J + 3, cross(arm, r));
    if (two) {
        const V3<T> g = cross(a2, r);
        J[6] = -r.x; J[7] = -r.y; J[8] = -r.z;
        J[9] = -g.x; J[10] = -g.y; J[11] = -g.z;
    } else {
        for (int j = 6; j < 12; j++) J[j] = T(0);
    }
}

// The slider's linear unit, two rows.  The unit's reals: cpos / cnormal = the two sides' anchors (as a ball unit's), cbounce /
// cbounce_vel / csoft_erp = axis1 in the frame of body 1 (canonical sides).  u = R_1 axis1, r = p, q of plane_space(u):
// J = [ r, (p_2 - x_1) x r | -r, -(a_2 x r) ], c = k (p_2 - p_1) . r; p_2 - x_1 = a_1 + (p_2 - p_1).
template <class T>
DMX_HD int slider_unit_rows(const T *S, int64_t stride, const IslandSet<T> &I, const StepParams<T> &P, T *rows, int *jb, int ci, int m, T hinv)
{
    const int s1 = I.cb1[ci], s2 = I.cb2[ci];
    const int l1 = I.local[s1], l2 = s2 >= 0 ? I.local[s2] : -1;
    const M3<T> R1 = quat_to_R(ldq(S, s1));
    V3<T> a1, a2, err;
    slider_arms(S, stride, I, ci, R1, a1, a2, err);
    const V3<T> axis1 = { I.cbounce[ci], I.cbounce_vel[ci], I.csoft_erp[ci] };
    V3<T> dir[2];
    plane_space(mulv(R1, axis1), dir[0], dir[1]);
    const V3<T> arm = { a1.x + err.x, a1.y + err.y, a1.z + err.z };
    const T k = hinv * P.erp;
    for (int dnum = 0; dnum < 2; dnum++) {
        T *row = rows + (size_t)(m + dnum) * RW_COUNT;
        jb[2 * (m + dnum)] = l1; jb[2 * (m + dnum) + 1] = l2;
        slider_row_J(row + RW_J, dir[dnum], arm, a2, s2 >= 0);
        row[RW_LO] = -Limits<T>::inf(); row[RW_HI] = Limits<T>::inf();
        row[RW_RHS] = k * dot(err, dir[dnum]);      // c for now
        row[RW_AD] = P.cfm;                         // cfm for now
        row[RW_LAM] = T(0);
    }
    return 2;
}

// c, lo, hi of a limit / motor row from its coordinate (a hinge's theta, a slider's s): the table of include/dmx_batch.h
template <class T> DMX_HD void limot_table(T x, T lo_s, T hi_s, T vel, T fmax, T k, T &c, T &lo, T &hi)
{
    const T inf = Limits<T>::inf();
    const T g = fmax > T(0) ? (vel > T(0) ? fmax : vel < T(0) ? -fmax : T(0)) : T(0);
    const bool limited = lo_s <= hi_s && (lo_s > -inf || hi_s < inf);
    c = T(0); lo = T(0); hi = T(0);                        // inside its range, no motor: the row stays, and does nothing
    if (limited && lo_s == hi_s) { c = -k * (x - lo_s); lo = -inf; hi = inf; }
    else if (limited && x <= lo_s) { c = -k * (x - lo_s); lo = g; hi = inf; }
    else if (limited && x >= hi_s) { c = -k * (x - hi_s); lo = -inf; hi = g; }
    else if (fmax > T(0)) { c = vel; lo = -fmax; hi = fmax; }
}

// The slider limot's one row, behind the slider's five: the entry directly before it is the joint's linear unit (the host emits a
// joint's units back to back), whose anchors it reads.  Its own reals: cpos = axis1 AS GIVEN, cbounce / cbounce_vel / csoft_erp /
// csoft_cfm = lo_stop / hi_stop / vel / fmax; cmode != 0: the sides were exchanged.  With w = u = R_1 axis1 -- or, after an exchange
// (given side 1 is the world: u = its axis as given, and there is no body 2), w = -u -- in canonical sides s = -w . (p_2 - p_1) and
// J = [ w, arm x w | -w, -(a_2 x w) ], arm = p_2 - x_1 (after an exchange a_1): the row's velocity is s_dot.
template <class T>
DMX_HD int slimot_unit_row(const T *S, int64_t stride, const IslandSet<T> &I, const StepParams<T> &P, T *rows, int *jb, int ci, int m, T hinv)
{
    const int s1 = I.cb1[ci], s2 = I.cb2[ci];
    const bool rev = I.cmode[ci] != 0;
    T *row = rows + (size_t)m * RW_COUNT;
    jb[2 * m] = I.local[s1]; jb[2 * m + 1] = s2 >= 0 ? I.local[s2] : -1;
    const M3<T> R1 = quat_to_R(ldq(S, s1));
    V3<T> a1, a2, err;
    slider_arms(S, stride, I, ci - 1, R1, a1, a2, err);
    const V3<T> axis1 = ld3(I.cpos + 3 * (size_t)ci);
    V3<T> w = { -axis1.x, -axis1.y, -axis1.z }, arm = a1;
    if (!rev) { w = mulv(R1, axis1); arm = { a1.x + err.x, a1.y + err.y, a1.z + err.z }; }
    T c, lo, hi;
    limot_table(-dot(w, err), I.cbounce[ci], I.cbounce_vel[ci], I.csoft_erp[ci], I.csoft_cfm[ci], hinv * P.erp, c, lo, hi);
    row[RW_LO] = lo; row[RW_HI] = hi;
    row[RW_RHS] = c;                    // c for now
    row[RW_AD] = P.cfm;                 // cfm for now
    row[RW_LAM] = T(0);
    slider_row_J(row + RW_J, w, arm, a2, s2 >= 0);
    return 1;
}

// s and s_dot of a slider in the sides AS GIVEN (dmxBatchSliderPositions, the ODE face's dJointGetSliderPosition / Rate): has_i =
// side i is a body with position x_i, quaternion q_i, velocities v_i, w_i; anchor_i, axis1 in the side's frame (the world's when it
// is the world).  s = u . (p_1 - p_2), s_dot = [ u, (p_2 - x_1) x u | -u, -(a_2 x u) ] . (v_1, w_1, v_2, w_2).
template <class T>
DMX_HD void slider_position(bool has1, const V3<T> &x1, const Q4<T> &q1, const V3<T> &v1, const V3<T> &w1,
                            bool has2, const V3<T> &x2, const Q4<T> &q2, const V3<T> &v2, const V3<T> &w2,
                            const V3<T> &anchor1, const V3<T> &anchor2, const V3<T> &axis1, T &s, T &s_dot)
{
    V3<T> u = axis1, a1 = { T(0), T(0), T(0) }, a2 = a1, c1 = anchor1, c2 = anchor2;
    if (has1) { const M3<T> R = quat_to_R(q1); u = mulv(R, axis1); a1 = mulv(R, anchor1); c1 = x1; }
    if (has2) { a2 = mulv(quat_to_R(q2), anchor2); c2 = x2; }
    const V3<T> err = { diff_of_sums(c2.x, a2.x, c1.x, a1.x), diff_of_sums(c2.y, a2.y, c1.y, a1.y), diff_of_sums(c2.z, a2.z, c1.z, a1.z) };
    s = -dot(u, err);
    s_dot = T(0);
    if (has1) { const V3<T> arm = { a1.x + err.x, a1.y + err.y, a1.z + err.z }; s_dot = dot(u, v1) + dot(cross(arm, u), w1); }
    if (has2) s_dot -= dot(u, v2) + dot(cross(a2, u), w2);
}

// One axis of an angular motor (include/dmx_batch.h at DMX_JOINT_AMOTOR), one row.  Its geometry was made in front of the tick
// (amotor_prepare, dmx_artic.hip: no rotation and no atan2 here -- these kernels have no registers for them): cmode >> 1 = where the
// axis's prepared reals (dmx_amotor.hpp: a_i in the sides AS GIVEN, theta_i, then c, lo, hi) stand in I.amotor; cmode & 1: the sides
// were exchanged.  c, lo, hi are limot_table's, worked out by the prepare pass with the k = ERP / h this kernel would use: called
// from here the table cost five island kernels scratch (profiles/amotor_kernel_resources.txt).  (The entry's four surface slots are zero.)  In the sides as given J = [ 0, a_i | 0, -a_i ].
template <class T>
DMX_HD int amotor_unit_row(const IslandSet<T> &I, const StepParams<T> &P, T *rows, int *jb, int ci, int m, T hinv)
{
    const int s1 = I.cb1[ci], s2 = I.cb2[ci];
    const int cm = I.cmode[ci];
    T *row = rows + (size_t)m * RW_COUNT;
    jb[2 * m] = I.local[s1]; jb[2 * m + 1] = s2 >= 0 ? I.local[s2] : -1;
    const T *prep = I.amotor + (size_t)(cm >> 1);
    row[RW_LO] = prep[AMP_LO]; row[RW_HI] = prep[AMP_HI];
    row[RW_RHS] = prep[AMP_C];          // c for now
    row[RW_AD] = P.cfm;                 // cfm for now
    row[RW_LAM] = T(0);
    V3<T> u = ld3(prep + AMP_AXIS);
    if (cm & 1) u = { -u.x, -u.y, -u.z };      // (this entry's body 1 is the given body 2)
    T *J = row + RW_J;
    J[0] = J[1] = J[2] = T(0);
    st3(J + 3, u);
    for (int j = 6; j < 12; j++) J[j] = T(0);
    if (s2 >= 0) { J[9] = -u.x; J[10] = -u.y; J[11] = -u.z; }
    return 1;
}

// the slider's two linear units and an angular motor's unit, by marker (all at or below UNIT_SLIDER2_MU: contact_rows and
// joint_unit_rows send them here with the one comparison they always made)
template <class T>
DMX_HD int slider_linear_unit_rows(const T *S, int64_t stride, const IslandSet<T> &I, const StepParams<T> &P, T *rows, int *jb, int ci, int m, T hinv)
{
    const T mu = I.cmu[ci];
    if (mu == T(UNIT_SLIDER2_MU)) return slider_unit_rows(S, stride, I, P, rows, jb, ci, m, hinv);
    if (mu == T(UNIT_AMOTOR_MU)) return amotor_unit_row(I, P, rows, jb, ci, m, hinv);
    return slimot_unit_row(S, stride, I, P, rows, jb, ci, m, hinv);
}

// ---- rows of a unit of an articulation joint (dmxBatchSetJoints), written at island-relative row m ---------------------------
// The unit's six reals travel in the contact arrays: cpos = the first side's anchor (ball unit) or axis (hinge unit) in the
// frame of body 1, cnormal = the second side's in the frame of body 2 -- or in the world frame when there is no body 2.
//   ball unit, d = e_x, e_y, e_z:  J = [ d, a1 x d | -d, -(a2 x d) ],  c = k ((x2 + a2) - (x1 + a1)) . d,   a_i = R_i anchor_i
//   hinge unit, r = p, q of plane_space(u), u = R_1 axis1, w = R_2 axis2:  J = [ 0, r | 0, -r ],  c = k (u x w) . r
//   lock unit (slider, fixed), d = e_x, e_y, e_z:  J = [ 0, d | 0, -d ],  c = k Phi . d,  Phi = R_1 (2 e_v), e = conj(q_1) q_2 conj(q_0c):
//     cnormal + cdepth = q_0c (w, x, y, z).  It is built here, as a variant of the hinge unit, and not in a function of its own:
//     that costs solve_islands<float> eleven VGPRs and a wave per SIMD (profiles/slider_kernel_resources.txt)
// with k = erp / h, cfm = the world's, no bounds.  (A limot unit: limot_unit_row; a slider's linear and limot units:
// slider_linear_unit_rows.)  Returns the unit's row count.
template <class T>
DMX_HD int joint_unit_rows(const T *S, int64_t stride, const IslandSet<T> &I, const StepParams<T> &P,
                                               T *rows, int *jb, int ci, int m, T hinv)
{
    // (for callers outside the kernels -- the host harnesses.  The kernels come through contact_rows, which sends a limot unit to
    //  limot_unit_row itself and never gets here with one: dispatched only from here, solve_islands<float> needs 82 VGPRs for 80 and
    //  loses its sixth wave per SIMD, profiles/limot_kernel_resources.txt.  Keep both.)
    if (I.cmu[ci] == T(UNIT_LIMOT_MU)) return limot_unit_row(S, I, P, rows, jb, ci, m, hinv);
    if (I.cmu[ci] <= T(UNIT_SLIDER2_MU)) return slider_linear_unit_rows(S, stride, I, P, rows, jb, ci, m, hinv);
    const int s1 = I.cb1[ci], s2 = I.cb2[ci];
    const int l1 = I.local[s1], l2 = s2 >= 0 ? I.local[s2] : -1;
    const bool hinge2 = I.cmu[ci] == T(UNIT_HINGE2_MU), lock = I.cmu[ci] == T(UNIT_LOCK_MU);
    V3<T> f1 = ld3(I.cpos + 3 * (size_t)ci);
    const V3<T> f2 = ld3(I.cnormal + 3 * (size_t)ci);
    const Q4<T> q1 = { S[slab_ix(C_QUAT + 0, s1)], S[slab_ix(C_QUAT + 1, s1)], S[slab_ix(C_QUAT + 2, s1)], S[slab_ix(C_QUAT + 3, s1)] };
    if (lock) {
        // the angular-lock unit of a slider or a fixed joint: cnormal[3] + cdepth = q_0c, the zero pose in canonical sides; what
        // is turned into the world frame below is 2 e_v of e = conj(q_1) q_2 conj(q_0c)
        Q4<T> q2 = { T(1), T(0), T(0), T(0) };
        if (s2 >= 0) q2 = ldq(S, s2);
        const Q4<T> q0 = { f2.x, f2.y, f2.z, I.cdepth[ci] };
        f1 = lock_error(pose_error(q1, q2, q0));
    }
    const V3<T> w1 = mulv(quat_to_R(q1), f1);              // a1 (ball unit) / u (hinge unit) / Phi (lock unit)
    V3<T> w2 = f2;                                         // a world side: the anchor / axis as given
    if (s2 >= 0 && !lock) {
        const Q4<T> q2 = { S[slab_ix(C_QUAT + 0, s2)], S[slab_ix(C_QUAT + 1, s2)], S[slab_ix(C_QUAT + 2, s2)], S[slab_ix(C_QUAT + 3, s2)] };
        w2 = mulv(quat_to_R(q2), f2);
    }
    const T k = hinv * P.erp;
    V3<T> dir[3], err;
    int n;
    if (hinge2) {
        n = 2;
        plane_space(w1, dir[0], dir[1]);
        dir[2] = { T(0), T(0), T(0) };
        err = cross(w1, w2);
    } else if (lock) {
        n = 3;
        dir[0] = { T(1), T(0), T(0) }; dir[1] = { T(0), T(1), T(0) }; dir[2] = { T(0), T(0), T(1) };
        err = w1;
    } else {
        n = 3;
        dir[0] = { T(1), T(0), T(0) }; dir[1] = { T(0), T(1), T(0) }; dir[2] = { T(0), T(0), T(1) };
        const V3<T> x1 = ldS(S, stride, C_POS, s1);
        // (x2 + a2) - (x1 + a1); a world side's point is its anchor (x = anchor, a = 0).  The four terms cancel to the joint's
        // error, which ERP / h carries straight into the velocities: summed plainly, the rounding of x + a -- an ulp of the
        // POSITIONS -- would come out as 12 ulp(x) of velocity noise at h = 1/60.  (x2 - x1) + (a2 - a1) with the sums' rounding
        // errors carried along (two_sum) is exact to an ulp of the error itself.
        V3<T> x2 = w2, a2 = { T(0), T(0), T(0) };
        if (s2 >= 0) { x2 = ldS(S, stride, C_POS, s2); a2 = w2; }
        err = { diff_of_sums(x2.x, a2.x, x1.x, w1.x), diff_of_sums(x2.y, a2.y, x1.y, w1.y), diff_of_sums(x2.z, a2.z, x1.z, w1.z) };
    }
    for (int dnum = 0; dnum < n; dnum++) {
        T *row = rows + (size_t)(m + dnum) * RW_COUNT;
        jb[2 * (m + dnum)] = l1; jb[2 * (m + dnum) + 1] = l2;
        T *J = row + RW_J;
        const V3<T> d = dir[dnum];
        const V3<T> zero = { T(0), T(0), T(0) };
        const bool angular = hinge2 || lock;
        const V3<T> lin = angular ? zero : d;
        const V3<T> ang1 = angular ? d : cross(w1, d);
        st3(J, lin);
        st3(J + 3, ang1);
        if (s2 >= 0) {
            const V3<T> ang2 = angular ? d : cross(w2, d);
            J[6] = -lin.x; J[7] = -lin.y; J[8] = -lin.z;
            J[9] = -ang2.x; J[10] = -ang2.y; J[11] = -ang2.z;
        } else {
            for (int j = 6; j < 12; j++) J[j] = T(0);
        }
        row[RW_LO] = -Limits<T>::inf(); row[RW_HI] = Limits<T>::inf();
        row[RW_RHS] = k * dot(err, d);      // c for now
        row[RW_AD] = P.cfm;                 // cfm for now
        row[RW_LAM] = T(0);
    }
    return n;
}

// ---- contact_rows with the second body absent, for the one-lane forms of a one-body island (dmx_islands_dev.hpp), which keep their
// rows in storage of their own; held to contact_rows bit for bit by tests/harness/single_contact_harness.cpp.  Contact ci of the body
// at x1: gi = its index in the table its geometry lies in, c1 = the contact point less x1, the surface mode, rows per contact, their
// directions (normal, then the two friction directions when mu > 0) and the friction rows' bounds.
template <class T>
DMX_HD void single_contact(const IslandSet<T> &I, const StepParams<T> &P, int ci, const V3<T> &x1, size_t &gi, V3<T> &c1, int &mode,
                           int &rpc, V3<T> *dir, T &lo_f, T &hi_f)
{
    const bool own_surface = I.cmu != nullptr, ind = I.csrc != nullptr;
    gi = ind ? (size_t)I.csrc[ci] : (size_t)ci;
    const V3<T> normal = ld3((ind ? I.gnormal : I.cnormal) + 3 * gi);
    const V3<T> cpos = ld3((ind ? I.gpos : I.cpos) + 3 * gi);
    c1 = { cpos.x - x1.x, cpos.y - x1.y, cpos.z - x1.z };
    mode = own_surface ? I.cmode[ci] : P.surf_mode;
    T mu = own_surface ? I.cmu[ci] : P.mu;
    if (mu < 0) mu = 0;
    rpc = mu > 0 ? 3 : 1;
    dir[0] = normal;
    dir[1] = dir[2] = { T(0), T(0), T(0) };
    if (rpc == 3) plane_space(normal, dir[1], dir[2]);
    lo_f = -mu; hi_f = mu;
}
// ... and its row along d: J = [d | c1 x d], c and cfm ("for now": row_setup divides by h) -- for the normal row the surface rule: soft
// ERP / CFM, depth less the surface layer, the maximum correcting velocity (dmxBatchSetContactCorrection), bounce
template <class T>
DMX_HD void single_contact_row(const IslandSet<T> &I, const StepParams<T> &P, int ci, size_t gi, int mode, bool is_normal, const V3<T> &c1,
                               const V3<T> &d, const V3<T> &v1, const V3<T> &w1, T hinv, T *J, T &cval, T &cfm)
{
    J[0] = d.x; J[1] = d.y; J[2] = d.z;
    const V3<T> a = cross(c1, d);
    J[3] = a.x; J[4] = a.y; J[5] = a.z;
    cval = T(0); cfm = P.cfm;
    if (!is_normal) return;
    const bool own_surface = I.cmu != nullptr;
    T erp = P.erp;
    if (mode & SURF_SOFT_ERP) erp = own_surface ? I.csoft_erp[ci] : T(0);
    if (mode & SURF_SOFT_CFM) cfm = own_surface ? I.csoft_cfm[ci] : T(0);
    T depth = (I.csrc != nullptr ? I.gdepth[gi] : I.cdepth[ci]) - I.surface_layer;
    if (depth < 0) depth = 0;
    cval = (hinv * erp) * depth;
    if (cval > I.max_corr_vel) cval = I.max_corr_vel;
    if (mode & SURF_BOUNCE) {
        const T outgoing = dot3p(J, v1) + dot3p(J + 3, w1);
        const T bv = own_surface ? I.cbounce_vel[ci] : P.bounce_vel;
        if (bv >= 0 && (-outgoing) > bv) {
            const T newc = -(own_surface ? I.cbounce[ci] : P.bounce) * outgoing;
            if (newc > cval) cval = newc;
        }
    }
}

// ---- rows of contact ci (normal + 2 friction when mu > 0), written at island-relative row m -----------------
// RPCK = 3: the caller knows the contact has friction rows (constant trip counts: a caller that hands in thread-local
// arrays gets them in registers)
// APX (a tick with at least one pyramid row, DMX_CONTACT_APPROX1: its own instantiation, as FB is): friction row d of a contact whose
// mode has DMX_CONTACT_APPROX1_d and whose mu is positive and finite is marked (RW_FMU, RW_FDIR) and built with lo = hi = 0 -- what
// dWorldStep's pass A solves; QuickStep's sweeps and dWorldStep's pass B make its bounds from the normal row's multiplier -- and
// every other row of the tick gets RW_FMU <= 0
// APX with I.cext set (an extended tick, dmxBatchStepJointsSurface; the definition: include/dmx_batch.h at DMX_CONTACT_MU2): a
// coefficient per friction row (mu_1, mu_2: all of the above with mu_d in place of mu; a row with mu_d = 0 is built with lo = hi = 0),
// d_1 = fdir1 and d_2 = n x d_1 where the contact's mode has DMX_CONTACT_FDIR1, c of the friction rows from motion1 / motion2 and
// motionN added to the normal row's before the cap, the friction rows' cfm from slip1 / slip2 -- all as the host staged them behind
// I.cext (dmx_internal.hpp at EXT_MU2).  With I.cext null, and in every instantiation without APX, the rows are what they were.
// (host too: tests/harness/friction_sweep_harness.cpp, tests/harness/surface_rows_harness.cpp)
template <class T, int RPCK = 0, bool APX = false>
DMX_HD void contact_rows(const T *S, int64_t stride, const IslandSet<T> &I, const StepParams<T> &P,
                                             T *rows, int *jb, int ci, int m, T hinv)
{
    if (RPCK == 0 && contact_is_unit(I, ci)) {
        if (I.cmu[ci] == T(UNIT_LIMOT_MU)) (void)limot_unit_row(S, I, P, rows, jb, ci, m, hinv);
        else if (I.cmu[ci] <= T(UNIT_SLIDER2_MU)) (void)slider_linear_unit_rows(S, stride, I, P, rows, jb, ci, m, hinv);
        else (void)joint_unit_rows(S, stride, I, P, rows, jb, ci, m, hinv);
        if (APX) for (int r = 0; r < unit_rows_of(I.cmu[ci]); r++) rows[(size_t)(m + r) * RW_COUNT + RW_FMU] = T(0);
        return;
    }
    const int s1 = I.cb1[ci], s2 = I.cb2[ci];
    const int l1 = I.local[s1], l2 = s2 >= 0 ? I.local[s2] : -1;
    const bool ind = I.csrc != nullptr;
    const size_t gi = ind ? (size_t)I.csrc[ci] : (size_t)ci;
    const V3<T> normal = ld3((ind ? I.gnormal : I.cnormal) + 3 * gi);
    const V3<T> cpos = ld3((ind ? I.gpos : I.cpos) + 3 * gi);
    const V3<T> x1 = ldS(S, stride, C_POS, s1);
    const V3<T> c1 = { cpos.x - x1.x, cpos.y - x1.y, cpos.z - x1.z };
    V3<T> c2 = { T(0), T(0), T(0) };
    if (s2 >= 0) {
        const V3<T> x2 = ldS(S, stride, C_POS, s2);
        c2 = { cpos.x - x2.x, cpos.y - x2.y, cpos.z - x2.z };
    }
    const bool own_surface = I.cmu != nullptr;
    const int mode = own_surface ? I.cmode[ci] : P.surf_mode;
    T mu = own_surface ? I.cmu[ci] : P.mu;
    if (mu < 0) mu = 0;
    const int rpc = RPCK ? RPCK : (mu > 0 ? 3 : 1);
    // the extended surface (an extended tick only: the pointer is a kernel argument, a wave-uniform test): mu_r per friction row,
    // and below the rows' directions, right-hand sides and CFM.  (cmu > 0 when either coefficient is: see SURF_EXT_MU1_ZERO.)
    const T *ext = nullptr;
    T mu1 = mu, mu2 = mu;
    if (APX) {
        if (I.cext != nullptr) {
            ext = I.cext + (size_t)EXT_REALS * (size_t)ci;
            if (mode & SURF_EXT_MU1_ZERO) mu1 = T(0);
            mu2 = ext[EXT_MU2];
        }
    }
    V3<T> dir[3];
    dir[0] = normal;
    if (rpc == 3) {
        if (APX && ext != nullptr && (mode & SURF_FDIR1)) { dir[1] = ld3(ext + EXT_FDIR1); dir[2] = cross(normal, dir[1]); }
        else plane_space(normal, dir[1], dir[2]);
    }
    // bit SURF_APPROX1_d: row d is a pyramid row
    int pyr = 0;
    if (APX && rpc == 3) {
        if (mu1 > 0 && mu1 < Limits<T>::inf()) pyr |= mode & SURF_APPROX1_1;
        if (mu2 > 0 && mu2 < Limits<T>::inf()) pyr |= mode & SURF_APPROX1_2;
    }
#pragma unroll
    for (int dnum = 0; dnum < rpc; dnum++) {
        T *row = rows + (size_t)(m + dnum) * RW_COUNT;
        jb[2 * (m + dnum)] = l1; jb[2 * (m + dnum) + 1] = l2;
        T *J = row + RW_J;
        st3(J, dir[dnum]);
        st3(J + 3, cross(c1, dir[dnum]));
        if (s2 >= 0) {
            J[6] = -dir[dnum].x; J[7] = -dir[dnum].y; J[8] = -dir[dnum].z;
            const V3<T> a = cross(c2, dir[dnum]);
            J[9] = -a.x; J[10] = -a.y; J[11] = -a.z;
        } else {
            for (int j = 6; j < 12; j++) J[j] = T(0);
        }
        T cval = T(0), cfm = P.cfm;
        if (dnum == 0) {
            // (single_contact_row's surface rule, spelt again with the second body's share of the approach speed: change both, the host
            //  harness above holds them together.  Taken from one function, eight kernels of dmx_lcp change: profiles/fused_dedup_resources.txt, section 2.)
            T erp = P.erp;
            if (mode & SURF_SOFT_ERP) erp = own_surface ? I.csoft_erp[ci] : T(0);
            if (mode & SURF_SOFT_CFM) cfm = own_surface ? I.csoft_cfm[ci] : T(0);
            T depth = (ind ? I.gdepth[gi] : I.cdepth[ci]) - I.surface_layer;      // (dmxBatchSetContactCorrection; 0 and +inf by default)
            if (depth < 0) depth = 0;
            cval = (hinv * erp) * depth;
            if (APX) { if (ext != nullptr) cval += ext[EXT_MOTIONN]; }
            if (cval > I.max_corr_vel) cval = I.max_corr_vel;
            if (mode & SURF_BOUNCE) {
                T outgoing = dot3p(J, ldS(S, stride, C_LVEL, s1)) + dot3p(J + 3, ldS(S, stride, C_AVEL, s1));
                if (s2 >= 0) outgoing += dot3p(J + 6, ldS(S, stride, C_LVEL, s2)) + dot3p(J + 9, ldS(S, stride, C_AVEL, s2));
                const T bv = own_surface ? I.cbounce_vel[ci] : P.bounce_vel;
                if (bv >= 0 && (-outgoing) > bv) {
                    const T newc = -(own_surface ? I.cbounce[ci] : P.bounce) * outgoing;
                    if (newc > cval) cval = newc;
                }
            }
            row[RW_LO] = T(0); row[RW_HI] = Limits<T>::inf();
            if (APX) row[RW_FMU] = pyr ? T(-1) : T(0);
        } else {
            const T mud = APX ? (dnum == 1 ? mu1 : mu2) : mu;
            row[RW_LO] = -mud; row[RW_HI] = mud;
            if (APX) {
                const bool p = (pyr & (SURF_APPROX1_1 << (dnum - 1))) != 0;
                if (p) { row[RW_LO] = T(0); row[RW_HI] = T(0); }
                row[RW_FMU] = p ? mud : T(0); row[RW_FDIR] = T(dnum);
                if (ext != nullptr) {
                    cval = ext[EXT_MOTION1 + dnum - 1];
                    const T slip = ext[EXT_SLIP1 + dnum - 1];
                    if (slip >= 0) cfm = slip;
                }
            }
        }
        row[RW_RHS] = cval;     // c for now
        row[RW_AD] = cfm;       // cfm for now
        row[RW_LAM] = T(0);
    }
}

// ---- v/h + M^-1 f of body k ------------------------------------------------------------------------------------
template <class T>
DMX_HD void body_tmp(const T *S, int64_t stride, T *b, int s, T hinv)
{
    const T im = b[BW_INVM];
    const V3<T> v = ldS(S, stride, C_LVEL, s), w = ldS(S, stride, C_AVEL, s);
    b[BW_TMP + 0] = fma_(b[BW_FACC + 0], im, v.x * hinv);
    b[BW_TMP + 1] = fma_(b[BW_FACC + 1], im, v.y * hinv);
    b[BW_TMP + 2] = fma_(b[BW_FACC + 2], im, v.z * hinv);
    const V3<T> tacc = ld3(b + BW_TACC);
    b[BW_TMP + 3] = dot3p(b + BW_INVI + 0, tacc);
    b[BW_TMP + 4] = dot3p(b + BW_INVI + 3, tacc);
    b[BW_TMP + 5] = dot3p(b + BW_INVI + 6, tacc);
    b[BW_TMP + 3] = fma_(w.x, hinv, b[BW_TMP + 3]); b[BW_TMP + 4] = fma_(w.y, hinv, b[BW_TMP + 4]);
    b[BW_TMP + 5] = fma_(w.z, hinv, b[BW_TMP + 5]);
}

// ---- row i: rhs = c/h - J (v/h + M^-1 f); cfm /= h; iMJ = M^-1 J^T; Ad = w/(J iMJ + cfm); J *= Ad; rhs *= Ad; Ad *= cfm
// SOR = false (the exact solve of dWorldStep): stop after iMJ -- J and rhs stay unscaled, row[RW_AD] = cfm / h
// FB (a launch made with feedback on: its own instantiation, so that the others are compiled as if it did not exist): the scaled form
// also stores Ad in the spare slot RW_UNSCALE, for entry_feedback
// (host too: tests/harness/feedback_rows_harness.cpp)
template <class T, bool SOR = true, bool FB = false>
DMX_HD void row_setup(T *rows, const int *jb, const T *bs, int i, T hinv, T sor_w)
{
    T *row = rows + (size_t)i * RW_COUNT;
    T *J = row + RW_J, *iMJ = row + RW_IMJ;
    const int l1 = jb[2 * i], l2 = jb[2 * i + 1];
    T sum = T(0);
    const T *in = bs + (size_t)l1 * BW_COUNT + BW_TMP;
    for (int j = 0; j < 6; j++) sum = fma_(J[j], in[j], sum);
    if (l2 >= 0) {
        in = bs + (size_t)l2 * BW_COUNT + BW_TMP;
        for (int j = 0; j < 6; j++) sum = fma_(J[6 + j], in[j], sum);
    }
    row[RW_RHS] = fma_(row[RW_RHS], hinv, -sum);
    row[RW_AD] *= hinv;

    const T *b1 = bs + (size_t)l1 * BW_COUNT;
    for (int j = 0; j < 3; j++) iMJ[j] = b1[BW_INVM] * J[j];
    const V3<T> ja1 = ld3(J + 3);
    iMJ[3] = dot3p(b1 + BW_INVI + 0, ja1); iMJ[4] = dot3p(b1 + BW_INVI + 3, ja1); iMJ[5] = dot3p(b1 + BW_INVI + 6, ja1);
    if (l2 >= 0) {
        const T *b2 = bs + (size_t)l2 * BW_COUNT;
        for (int j = 0; j < 3; j++) iMJ[6 + j] = b2[BW_INVM] * J[6 + j];
        const V3<T> ja2 = ld3(J + 9);
        iMJ[9] = dot3p(b2 + BW_INVI + 0, ja2); iMJ[10] = dot3p(b2 + BW_INVI + 3, ja2); iMJ[11] = dot3p(b2 + BW_INVI + 6, ja2);
    } else {
        for (int j = 6; j < 12; j++) iMJ[j] = T(0);
    }
    if (!SOR) return;
    T s2 = T(0);
    for (int j = 0; j < 6; j++) s2 = fma_(iMJ[j], J[j], s2);
    if (l2 >= 0) for (int j = 6; j < 12; j++) s2 = fma_(iMJ[j], J[j], s2);
    const T cfm = row[RW_AD];
    const T ad = sor_w / (s2 + cfm);
    for (int j = 0; j < 12; j++) J[j] *= ad;
    row[RW_RHS] *= ad;
    row[RW_AD] = ad * cfm;
    if (FB) row[RW_UNSCALE] = ad;
}

// ---- feedback (dmxBatchSetFeedback; the definition: include/dmx_batch.h) ---------------------------------------------------------
// acc[0..12) += sum over the rows of entry ci (a contact, or a unit of an articulation joint) of lambda_r J_r, J_r as the builders
// made it: [Jl1, Ja1 | Jl2, Ja2] in the entry's own (canonical) sides.  rows = the island's rows; the entry's first row is
// crow[ci], its row count comes from its kind.  scaled: the rows went through QuickStep's row_setup<T, true, FB = true> -- J holds J Ad
// and RW_UNSCALE holds Ad, so lambda_r J_r = (lambda_r / Ad) (J_r Ad).  Neither M^-1 J^T (zero for a kinematic body) nor
// RW_AD (Ad cfm: cfm may be zero) could give J back.  A world side's block is zero as built.
template <class T>
DMX_HD void entry_feedback(const IslandSet<T> &I, const StepParams<T> &P, const T *rows, int ci, bool scaled, T *acc)
{
    const T mu = I.cmu != nullptr ? I.cmu[ci] : P.mu;
    const int n = (I.has_units && mu < 0) ? unit_rows_of(mu) : (mu > 0 ? 3 : 1);
    const T *row = rows + (size_t)I.crow[ci] * RW_COUNT;
    for (int r = 0; r < n; r++, row += RW_COUNT) {
        const T l = scaled ? row[RW_LAM] / row[RW_UNSCALE] : row[RW_LAM];
        for (int j = 0; j < 12; j++) acc[j] = fma_(l, row[RW_J + j], acc[j]);
    }
}
// The feedback of the joint whose first entry is ci: the sum over its entries (info >> 1 of them, adjacent), in the sides AS GIVEN
// (info & 1: the entry's sides are the given ones exchanged) -> out[0..12) = f1, t1, f2, t2.
template <class T>
DMX_HD void joint_feedback(const IslandSet<T> &I, const StepParams<T> &P, const T *rows, int ci, int info, bool scaled, T *out)
{
    T acc[12];
    for (int j = 0; j < 12; j++) acc[j] = T(0);
    for (int u = 0; u < (info >> 1); u++) entry_feedback(I, P, rows, ci + u, scaled, acc);
    const int sw = (info & 1) ? 6 : 0;
    for (int j = 0; j < 6; j++) { out[j] = acc[j + sw]; out[6 + j] = acc[6 + j - sw]; }
}

// ---- one SOR row update; returns |delta lambda| -----------------------------------------------------------------
// The bounds of a pyramid row (RW_FMU > 0) when a sweep visits it: -/+ |mu lambda_n|, lambda_n = the multiplier of its contact's normal
// row as it stands (rows in creation order: already updated in this sweep).  One spelling for every SOR form.
template <class T> DMX_HD void pyramid_bounds(T fmu, T lam_n, T &lo, T &hi)
{
    hi = tabs(fmu * lam_n);
    lo = -hi;
}
// APX: see contact_rows (host too: tests/harness/friction_sweep_harness.cpp)
template <class T, bool APX = false>
DMX_HD T row_sor(T *rows, const int *jb, T *bs, int i)
{
    T *row = rows + (size_t)i * RW_COUNT;
    const T *J = row + RW_J, *iMJ = row + RW_IMJ;
    const int l1 = jb[2 * i], l2 = jb[2 * i + 1];
    T *fc1 = bs + (size_t)l1 * BW_COUNT + BW_FC;
    T *fc2 = l2 >= 0 ? bs + (size_t)l2 * BW_COUNT + BW_FC : nullptr;
    const T old = row[RW_LAM];
    T delta = fma_(-old, row[RW_AD], row[RW_RHS]);
    delta -= fma_(fc1[5], J[5], fma_(fc1[4], J[4], fma_(fc1[3], J[3], fma_(fc1[2], J[2], fma_(fc1[1], J[1], fc1[0] * J[0])))));
    if (fc2)
        delta -= fma_(fc2[5], J[11], fma_(fc2[4], J[10], fma_(fc2[3], J[9], fma_(fc2[2], J[8], fma_(fc2[1], J[7], fc2[0] * J[6])))));
    T lo = row[RW_LO], hi = row[RW_HI];
    if (APX) {
        const T fmu = row[RW_FMU];
        if (fmu > T(0)) pyramid_bounds(fmu, rows[(size_t)(i - (int)row[RW_FDIR]) * RW_COUNT + RW_LAM], lo, hi);
    }
    const T nl = old + delta;
    if (nl < lo) { delta = lo - old; row[RW_LAM] = lo; }
    else if (nl > hi) { delta = hi - old; row[RW_LAM] = hi; }
    else row[RW_LAM] = nl;
    for (int j = 0; j < 6; j++) fc1[j] = fma_(delta, iMJ[j], fc1[j]);
    if (fc2) for (int j = 0; j < 6; j++) fc2[j] = fma_(delta, iMJ[6 + j], fc2[j]);
    return tabs(delta);
}

// ---- the same row update with the row in registers and the bodies' constraint-force accumulators in LDS
//      (solve_island_wg): identical arithmetic, identical bits ---------------------------------------------------
// workgroup barrier that orders LDS traffic only (see solve_island_wg's level loop)
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__) && !defined(__gfx942__) && !defined(__gfx90a__)
#error "lds_barrier() spells gfx9's s_waitcnt lgkmcnt(0) + s_barrier: this library is written for gfx950 (csrc/Makefile ARCH)"
#endif
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <class T> struct RowRegs { T J[12], iMJ[12], rhs, ad, lo, hi, lam; int l1, l2, row; };

template <class T>
__device__ __forceinline__ void row_load(const T *rows, const int *jb, int i, RowRegs<T> &r)
{
    // the whole row as 16-byte pieces (rows are aligned to their own size: ISLAND_ROW_REALS reals from an aligned base)
    constexpr int PER = 16 / (int)sizeof(T), NP = RW_COUNT / PER;
    struct alignas(16) Piece { T v[PER]; };
    const Piece *row = reinterpret_cast<const Piece *>(rows + (size_t)i * RW_COUNT);
    T f[RW_COUNT];
#pragma unroll
    for (int p = 0; p < NP; p++) {
        const Piece q = row[p];
#pragma unroll
        for (int e = 0; e < PER; e++) f[p * PER + e] = q.v[e];
    }
#pragma unroll
    for (int j = 0; j < 12; j++) { r.J[j] = f[RW_J + j]; r.iMJ[j] = f[RW_IMJ + j]; }
    r.rhs = f[RW_RHS]; r.ad = f[RW_AD]; r.lo = f[RW_LO]; r.hi = f[RW_HI]; r.lam = f[RW_LAM];
    const int2 b = *reinterpret_cast<const int2 *>(jb + 2 * (size_t)i);
    r.l1 = b.x; r.l2 = b.y;
    r.row = i;
}

template <class T, bool STORE_LAM = true>
__device__ __forceinline__ T row_sor_lds(T *rows, RowRegs<T> &r, T *fc, bool eager = true)
{
    // both bodies' accumulators are fetched together, up front, and written back from registers: the row's two bodies differ,
    // so nothing needs re-reading in between -- one LDS round trip per row instead of three.  eager: a body-less second slot
    // fetches too (the first body's values, never used), which keeps the two fetches in one straight line of code; launches
    // of thousands of islands are bound by issue slots, not by latency, and fetch only what they use.
    T *fc1 = fc + 6 * r.l1;
    T *fc2 = fc + 6 * (r.l2 >= 0 ? r.l2 : r.l1);
    const bool two = r.l2 >= 0;
    T a[6], b[6];
#pragma unroll
    for (int j = 0; j < 6; j++) a[j] = fc1[j];
    if (two || eager) {
#pragma unroll
        for (int j = 0; j < 6; j++) b[j] = fc2[j];
    } else {
#pragma unroll
        for (int j = 0; j < 6; j++) b[j] = T(0);
    }
    const T *J = r.J;
    const T old = r.lam;
    T delta = fma_(-old, r.ad, r.rhs);
    delta -= fma_(a[5], J[5], fma_(a[4], J[4], fma_(a[3], J[3], fma_(a[2], J[2], fma_(a[1], J[1], a[0] * J[0])))));
    if (two)
        delta -= fma_(b[5], J[11], fma_(b[4], J[10], fma_(b[3], J[9], fma_(b[2], J[8], fma_(b[1], J[7], b[0] * J[6])))));
    const T nl = old + delta;
    if (nl < r.lo) { delta = r.lo - old; r.lam = r.lo; }
    else if (nl > r.hi) { delta = r.hi - old; r.lam = r.hi; }
    else r.lam = nl;
    if (STORE_LAM) rows[(size_t)r.row * RW_COUNT + RW_LAM] = r.lam;
#pragma unroll
    for (int j = 0; j < 6; j++) fc1[j] = fma_(delta, r.iMJ[j], a[j]);
    if (two) {
#pragma unroll
        for (int j = 0; j < 6; j++) fc2[j] = fma_(delta, r.iMJ[6 + j], b[j]);
    }
    return tabs(delta);
}

// ---- body k: v += h cforce ; v += h M^-1 f ; integrate ; clear accumulators -------------------------------------
// (damping: IslandSet::damping, the per-slot table of dmx_damping.hpp or null -- the angular speed cap of a non-kinematic slot.
//  Every device caller names it: the form without it, below, exists on the host only)
template <class T>
DMX_HD void finish_body(T *S, const uint8_t *bflags, int64_t stride, const T *b, int s, bool has_rows, T h, const T *damping)
{
    V3<T> x = ldS(S, stride, C_POS, s);
    Q4<T> q = { S[slab_ix(C_QUAT + 0, s)], S[slab_ix(C_QUAT + 1, s)],
                S[slab_ix(C_QUAT + 2, s)], S[slab_ix(C_QUAT + 3, s)] };
    V3<T> v = ldS(S, stride, C_LVEL, s), w = ldS(S, stride, C_AVEL, s);
    if (has_rows) {
        v.x = fma_(h, b[BW_FC + 0], v.x); v.y = fma_(h, b[BW_FC + 1], v.y); v.z = fma_(h, b[BW_FC + 2], v.z);
        w.x = fma_(h, b[BW_FC + 3], w.x); w.y = fma_(h, b[BW_FC + 4], w.y); w.z = fma_(h, b[BW_FC + 5], w.z);
    }
    if (!(bflags[s] & BF_KINEMATIC)) {
        const T hm = h * b[BW_INVM];
        v.x = fma_(hm, b[BW_FACC + 0], v.x); v.y = fma_(hm, b[BW_FACC + 1], v.y); v.z = fma_(hm, b[BW_FACC + 2], v.z);
        V3<T> tacc = ld3(b + BW_TACC);
        tacc.x *= h; tacc.y *= h; tacc.z *= h;
        w.x += dot3p(b + BW_INVI + 0, tacc); w.y += dot3p(b + BW_INVI + 3, tacc); w.z += dot3p(b + BW_INVI + 6, tacc);
        // the angular speed cap, between the velocities and the poses (the quaternion advances with the capped avel); the table's
        // address is a kernel argument: a wave-uniform test, and nothing is loaded while the table does not exist
        if (damping != nullptr) cap_angular_speed(w, damping[(size_t)DAMP_REALS * (size_t)s + DAMP_MAX_ANG_SPEED]);
    }
    x.x = fma_(h, v.x, x.x); x.y = fma_(h, v.y, x.y); x.z = fma_(h, v.z, x.z);
    integrate_quat(q, w, h);
    S[slab_ix(C_POS + 0, s)] = x.x; S[slab_ix(C_POS + 1, s)] = x.y; S[slab_ix(C_POS + 2, s)] = x.z;
    S[slab_ix(C_QUAT + 0, s)] = q.w; S[slab_ix(C_QUAT + 1, s)] = q.x;
    S[slab_ix(C_QUAT + 2, s)] = q.y; S[slab_ix(C_QUAT + 3, s)] = q.z;
    S[slab_ix(C_LVEL + 0, s)] = v.x; S[slab_ix(C_LVEL + 1, s)] = v.y; S[slab_ix(C_LVEL + 2, s)] = v.z;
    S[slab_ix(C_AVEL + 0, s)] = w.x; S[slab_ix(C_AVEL + 1, s)] = w.y; S[slab_ix(C_AVEL + 2, s)] = w.z;
    for (int j = 0; j < 6; j++) S[slab_ix(C_FORCE + j, s)] = T(0);
}
// the integrator without a table, for the host harnesses that predate the cap (tests/harness/friction_sweep_harness.cpp): host
// only, so that a kernel that left the table out does not compile
template <class T>
__host__ inline void finish_body(T *S, const uint8_t *bflags, int64_t stride, const T *b, int s, bool has_rows, T h)
{
    finish_body<T>(S, bflags, stride, b, s, has_rows, h, (const T *)nullptr);
}

}  // namespace dmx
