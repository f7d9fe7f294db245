// dmx_artic.hip -- the articulation joints' entry points of the batch C ABI (include/dmx_batch.h): the persistent set
// (dmxBatchSetJoints), a joint from world-frame anchor and axis at the bodies' current poses (dmxBatchJointFromWorld), and the
// joints' position / axis errors from the current state, computed on the device (dmxBatchJointErrors); the hinges' limits and
// motors (dmxBatchSetHingeLimots, dmxBatchHingeLimotInit) and their angles and rates, computed on the device (dmxBatchHingeAngles),
// and the sliders' positions and rates (dmxBatchSliderPositions); the feedback of a tick's joints and contact joints (dmxBatchSetFeedback,
// dmxBatchJointFeedback, dmxBatchContactFeedback, dmxBatchFeedbackDevice) and the general path's kernel for it.
// The rows themselves are built by joint_unit_rows (dmx_island_rows.hpp) inside the island kernels; the host side of a tick is in
// dmx_joints.cpp.
#include <hip/hip_runtime.h>
#include <string.h>
#include <cmath>

#include "dmx_batch_priv.hpp"
#include "dmx_island_rows.hpp"
#include "dmx_amotor.hpp"

namespace dmx {

// One lane per joint: |p2 - p1| with p_i = x_i + R_i anchor_i (a world side: its anchor), and for hinges |u x w| with
// u = R_1 axis1, w = R_2 axis2; for a slider the part of p2 - p1 across its axis, and for sliders and fixed joints |2 e_v|, e = conj(q_1)
// q_2 conj(q_0) (limots null: q_0 the identity) -- the quantities the rows' right-hand sides pull to zero, in the batch's precision.  The two
// maxima: a wave reduction, then one atomic per wavefront on the values' bit patterns (non-negative doubles order like their bits).
template <class T>
__global__ __launch_bounds__(256) void joint_errors(const T *__restrict__ S, const uint8_t *__restrict__ bflags, int64_t stride, int64_t n_slots,
                                                    const dmxJoint *__restrict__ joints, const dmxHingeLimot *__restrict__ limots, int64_t nj,
                                                    double *__restrict__ pos_err, double *__restrict__ axis_err, unsigned long long *__restrict__ maxima)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double pe = 0.0, ae = 0.0;
    if (k < nj) {
        const dmxJoint j = joints[k];
        const int s1 = j.body1, s2 = j.body2;
        auto alive = [&](int s) { return s < n_slots && (bflags[s] & BF_ALIVE) != 0; };
        const bool active = !(s1 < 0 && s2 < 0) && s1 != s2 && (s1 < 0 || alive(s1)) && (s2 < 0 || alive(s2));
        if (active && j.kind != DMX_JOINT_AMOTOR) {       // (an angular motor has neither anchors nor an axis to be off: 0)
            auto side = [&](int s, const double *anchor, const double *axis, V3<T> &p, V3<T> &u) {
                const V3<T> a = { (T)anchor[0], (T)anchor[1], (T)anchor[2] }, ax = { (T)axis[0], (T)axis[1], (T)axis[2] };
                if (s < 0) { p = a; u = ax; return; }
                const Q4<T> q = { S[slab_ix(C_QUAT + 0, s)], S[slab_ix(C_QUAT + 1, s)], S[slab_ix(C_QUAT + 2, s)], S[slab_ix(C_QUAT + 3, s)] };
                const M3<T> R = quat_to_R(q);
                const V3<T> ra = mulv(R, a);
                p = { S[slab_ix(C_POS + 0, s)] + ra.x, S[slab_ix(C_POS + 1, s)] + ra.y, S[slab_ix(C_POS + 2, s)] + ra.z };
                u = mulv(R, ax);
            };
            V3<T> p1, p2, u, w;
            side(s1, j.anchor1, j.axis1, p1, u);
            side(s2, j.anchor2, j.axis2, p2, w);
            V3<T> d = { p2.x - p1.x, p2.y - p1.y, p2.z - p1.z };
            if (j.kind == DMX_JOINT_SLIDER) {
                // the part of p2 - p1 across the axis of side 1 (after an exchange of sides: of the given side 2)
                const V3<T> a = s1 >= 0 ? u : w;
                const T along = dot(d, a);
                d = { d.x - along * a.x, d.y - along * a.y, d.z - along * a.z };
            }
            pe = (double)tsqrt<T>(dot(d, d));
            if (j.kind == DMX_JOINT_HINGE) { const V3<T> c = cross(u, w); ae = (double)tsqrt<T>(dot(c, c)); }
            if (j.kind == DMX_JOINT_SLIDER || j.kind == DMX_JOINT_FIXED) {
                // |2 e_v| of e = conj(q_1) q_2 conj(q_0): the same for the sides as given and exchanged
                Q4<T> q0 = { T(1), T(0), T(0), T(0) }, q1 = q0, q2 = q0;
                if (limots != nullptr) q0 = { (T)limots[k].qrel0[0], (T)limots[k].qrel0[1], (T)limots[k].qrel0[2], (T)limots[k].qrel0[3] };
                if (s1 >= 0) q1 = ldq(S, s1);
                if (s2 >= 0) q2 = ldq(S, s2);
                const V3<T> c = lock_error(pose_error(q1, q2, q0));
                ae = (double)tsqrt<T>(dot(c, c));
            }
        }
        pos_err[k] = pe;
        axis_err[k] = ae;
    }
    double mp = pe, ma = ae;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double a = __shfl_xor(mp, o, 64), c = __shfl_xor(ma, o, 64);
        mp = a > mp ? a : mp;
        ma = c > ma ? c : ma;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMax(&maxima[0], (unsigned long long)__double_as_longlong(mp));
        atomicMax(&maxima[1], (unsigned long long)__double_as_longlong(ma));
    }
}

// One lane per joint: a hinge's theta (hinge_angle, the function the limot row is built with) and theta_dot = u . (omega_1 -
// omega_2), u = R_1 axis1, of the sides as given, in the batch's precision.  limots null: every q_0 is the identity.  Balls and
// inactive joints report 0.
template <class T>
__global__ __launch_bounds__(256) void hinge_angles(const T *__restrict__ S, const uint8_t *__restrict__ bflags, int64_t stride, int64_t n_slots,
                                                    const dmxJoint *__restrict__ joints, const dmxHingeLimot *__restrict__ limots, int64_t nj,
                                                    double *__restrict__ angle, double *__restrict__ rate)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nj) return;
    const dmxJoint j = joints[k];
    const int s1 = j.body1, s2 = j.body2;
    auto alive = [&](int s) { return s < n_slots && (bflags[s] & BF_ALIVE) != 0; };
    const bool active = !(s1 < 0 && s2 < 0) && s1 != s2 && (s1 < 0 || alive(s1)) && (s2 < 0 || alive(s2));
    double th = 0.0, thd = 0.0;
    if (active && j.kind == DMX_JOINT_HINGE) {
        Q4<T> q0 = { T(1), T(0), T(0), T(0) };
        if (limots != nullptr) q0 = { (T)limots[k].qrel0[0], (T)limots[k].qrel0[1], (T)limots[k].qrel0[2], (T)limots[k].qrel0[3] };
        auto quat = [&](int s) -> Q4<T> {
            if (s < 0) return { T(1), T(0), T(0), T(0) };
            return { S[slab_ix(C_QUAT + 0, s)], S[slab_ix(C_QUAT + 1, s)], S[slab_ix(C_QUAT + 2, s)], S[slab_ix(C_QUAT + 3, s)] };
        };
        auto omega = [&](int s) -> V3<T> {
            if (s < 0) return { T(0), T(0), T(0) };
            return { S[slab_ix(C_AVEL + 0, s)], S[slab_ix(C_AVEL + 1, s)], S[slab_ix(C_AVEL + 2, s)] };
        };
        const V3<T> axis1 = { (T)j.axis1[0], (T)j.axis1[1], (T)j.axis1[2] };
        const Q4<T> q1 = quat(s1);
        th = (double)hinge_angle(q1, quat(s2), q0, axis1);
        const V3<T> u = s1 >= 0 ? mulv(quat_to_R(q1), axis1) : axis1;
        const V3<T> w1 = omega(s1), w2 = omega(s2);
        const V3<T> dw = { w1.x - w2.x, w1.y - w2.y, w1.z - w2.z };
        thd = (double)dot(u, dw);
    }
    if (angle != nullptr) angle[k] = th;
    if (rate != nullptr) rate[k] = thd;
}

// One lane per joint: a slider's s and s_dot of the sides as given (slider_position, dmx_island_rows.hpp: what the limot row is
// built from), in the batch's precision.  Other kinds and inactive joints report 0.
template <class T>
__global__ __launch_bounds__(256) void slider_positions(const T *__restrict__ S, const uint8_t *__restrict__ bflags, int64_t stride, int64_t n_slots,
                                                        const dmxJoint *__restrict__ joints, int64_t nj, double *__restrict__ pos, double *__restrict__ rate)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nj) return;
    const dmxJoint j = joints[k];
    const int s1 = j.body1, s2 = j.body2;
    auto alive = [&](int s) { return s < n_slots && (bflags[s] & BF_ALIVE) != 0; };
    const bool active = !(s1 < 0 && s2 < 0) && s1 != s2 && (s1 < 0 || alive(s1)) && (s2 < 0 || alive(s2));
    T sp = T(0), sd = T(0);
    if (active && j.kind == DMX_JOINT_SLIDER) {
        const V3<T> zero = { T(0), T(0), T(0) };
        const Q4<T> ident = { T(1), T(0), T(0), T(0) };
        V3<T> x1 = zero, v1 = zero, w1 = zero, x2 = zero, v2 = zero, w2 = zero;
        Q4<T> q1 = ident, q2 = ident;
        if (s1 >= 0) { x1 = ldS(S, stride, C_POS, s1); q1 = ldq(S, s1); v1 = ldS(S, stride, C_LVEL, s1); w1 = ldS(S, stride, C_AVEL, s1); }
        if (s2 >= 0) { x2 = ldS(S, stride, C_POS, s2); q2 = ldq(S, s2); v2 = ldS(S, stride, C_LVEL, s2); w2 = ldS(S, stride, C_AVEL, s2); }
        const V3<T> an1 = { (T)j.anchor1[0], (T)j.anchor1[1], (T)j.anchor1[2] }, an2 = { (T)j.anchor2[0], (T)j.anchor2[1], (T)j.anchor2[2] };
        const V3<T> axis1 = { (T)j.axis1[0], (T)j.axis1[1], (T)j.axis1[2] };
        slider_position(s1 >= 0, x1, q1, v1, w1, s2 >= 0, x2, q2, v2, w2, an1, an2, axis1, sp, sd);
    }
    if (pos != nullptr) pos[k] = (double)sp;
    if (rate != nullptr) rate[k] = (double)sd;
}

// One lane per joint of the set: an active angular motor's three axes and three angles (amotor_axes) from the state as it stands --
// in front of a tick's first kernel on the tick's stream, that is the state at the tick's start -- into the table the island kernels'
// amotor_unit_row reads; every other joint's AMOTOR_PREP_REALS reals are zero.  rates (dmxBatchAMotorAngles only): a_i . (omega_1 - omega_2).
// The host has checked the records' slots against the batch's size.
template <class T>
__global__ __launch_bounds__(256) void amotor_prepare(const T *__restrict__ S, int64_t stride, const AMotorIn *__restrict__ in, int nj, T kerp,
                                                      T *__restrict__ prep, T *__restrict__ rates)
{
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= nj) return;
    V3<T> a[3];
    for (int i = 0; i < 3; i++) a[i] = { T(0), T(0), T(0) };
    const int s1 = in[k].body1, s2 = in[k].body2;
    const bool active = in[k].active != 0;
    T *o = prep + (size_t)AMOTOR_PREP_REALS * (size_t)k;
    if (active) {
        const Q4<T> ident = { T(1), T(0), T(0), T(0) };
        amotor_prepare_joint<T>(s1 >= 0, s1 >= 0 ? ldq(S, s1) : ident, s2 >= 0, s2 >= 0 ? ldq(S, s2) : ident, in[k].m, kerp, o, a);
    } else {
        for (int i = 0; i < AMOTOR_PREP_REALS; i++) o[i] = T(0);
    }
    if (rates != nullptr) {
        const V3<T> zero = { T(0), T(0), T(0) };
        const V3<T> w1 = active && s1 >= 0 ? ldS(S, stride, C_AVEL, s1) : zero, w2 = active && s2 >= 0 ? ldS(S, stride, C_AVEL, s2) : zero;
        const V3<T> dw = { w1.x - w2.x, w1.y - w2.y, w1.z - w2.z };
        for (int i = 0; i < 3; i++) rates[3 * (size_t)k + i] = dot(a[i], dw);
    }
}

template <class T>
hipError_t launch_amotor_prepare(const T *S, int64_t stride, const AMotorIn *in, int nj, T k, T *prep, T *rates, hipStream_t st)
{
    if (nj <= 0) return hipSuccess;
    hipLaunchKernelGGL((amotor_prepare<T>), dim3((unsigned)((nj + 255) / 256)), dim3(256), 0, st, S, stride, in, nj, k, prep, rates);
    return hipGetLastError();
}
template hipError_t launch_amotor_prepare<float>(const float *, int64_t, const AMotorIn *, int, float, float *, float *, hipStream_t);
template hipError_t launch_amotor_prepare<double>(const double *, int64_t, const AMotorIn *, int, double, double *, double *, hipStream_t);

// Feedback on the general path, behind the tick's solves on the tick's stream: one lane per entry of the contact arrays; the lane
// of a joint's first entry sums the joint's entries (they are adjacent), puts the sides back as given and writes the joint's 12
// reals.  Reads the row table and the tick's tables, writes F.fb; no atomics.  (The single-launch tick calls the same
// joint_feedback from inside its one kernel.)
template <class T>
__global__ __launch_bounds__(256) void joint_feedback_rows(IslandSet<T> I, StepParams<T> P, FeedbackSet<T> F, int n_entries)
{
    const int d = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (d >= n_entries) return;
    const int o = F.out[d];
    if (o < 0) return;
    const T *rows = I.rows + (size_t)I.row_off[F.isl[d]] * RW_COUNT;
    T out[12];
    joint_feedback(I, P, rows, d, F.info[d], F.mode == FB_SCALED, out);
#pragma unroll
    for (int j = 0; j < 12; j++) F.fb[(size_t)12 * o + j] = out[j];
}

template <class T>
hipError_t launch_feedback(const IslandSet<T> &I, const StepParams<T> &P, const FeedbackSet<T> &F, int n_entries, hipStream_t st)
{
    if (n_entries <= 0 || F.mode == FB_OFF) return hipSuccess;
    hipLaunchKernelGGL((joint_feedback_rows<T>), dim3((unsigned)((n_entries + 255) / 256)), dim3(256), 0, st, I, P, F, n_entries);
    return hipGetLastError();
}
template hipError_t launch_feedback<float>(const IslandSet<float> &, const StepParams<float> &, const FeedbackSet<float> &, int, hipStream_t);
template hipError_t launch_feedback<double>(const IslandSet<double> &, const StepParams<double> &, const FeedbackSet<double> &, int, hipStream_t);

}  // namespace dmx

extern "C" int dmxBatchSetFeedback(dmxBatchID b, int on)
{
    if (!b) return DMX_EINVAL;
    { const int rc = dmx_settle(b); if (rc != DMX_OK) return rc; }
    if ((on != 0) != b->fb_on) b->fb_valid = false;        // (switched on: no tick yet; switched off: nothing to serve)
    b->fb_on = on != 0;
    return DMX_OK;
}

// what the getters share: may the last tick's feedback be served at all?
static int feedback_ready(dmxBatch *b, const char *who)
{
    const char *why = !b->fb_on ? "feedback is off (dmxBatchSetFeedback)"
                    : !b->fb_valid ? "no dmxBatchStepJoints tick made with feedback on has run since the last other tick or dmxBatchSetJoints" : nullptr;
    if (why) { fprintf(stderr, "libode_mi355: %s: %s\n", who, why); return DMX_EINVAL; }
    return DMX_OK;
}
static int feedback_fetch(dmxBatch *b, int64_t first, int64_t count, dmxJointFeedback *out)
{
    if (count == 0) return DMX_OK;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipStreamSynchronize(b->stream));              // (the small tick's one wait, or the general path's kernel)
    const size_t rs = b->rsize;
    const void *src = b->fb_host ? (const void *)((const char *)b->fb_host + (size_t)12 * first * rs) : nullptr;
    if (!src) {
        b->fb_tmp.resize((size_t)12 * count * rs);
        HIP_TRY(hipMemcpy(b->fb_tmp.data(), (const char *)b->fb_devp + (size_t)12 * first * rs, (size_t)12 * count * rs, hipMemcpyDeviceToHost));
        src = b->fb_tmp.data();
    }
    double *o = (double *)out;
    static_assert(sizeof(dmxJointFeedback) == 12 * sizeof(double), "12 doubles, no padding");
    if (b->precision == DMX_F32) for (int64_t k = 0; k < 12 * count; k++) o[k] = (double)((const float *)src)[k];
    else memcpy(o, src, (size_t)12 * count * sizeof(double));
    return DMX_OK;
}

extern "C" int dmxBatchJointFeedback(dmxBatchID b, dmxJointFeedback *out)
{
    if (!b) return DMX_EINVAL;
    { const int rc = dmx_settle(b); if (rc != DMX_OK) return rc; }
    { const int rc = feedback_ready(b, "dmxBatchJointFeedback"); if (rc != DMX_OK) return rc; }
    if (b->fb_nj > 0 && !out) return DMX_EINVAL;
    return feedback_fetch(b, 0, b->fb_nj, out);
}

extern "C" int dmxBatchContactFeedback(dmxBatchID b, int64_t n, dmxJointFeedback *out)
{
    if (!b) return DMX_EINVAL;
    { const int rc = dmx_settle(b); if (rc != DMX_OK) return rc; }
    { const int rc = feedback_ready(b, "dmxBatchContactFeedback"); if (rc != DMX_OK) return rc; }
    if (n != b->fb_nc) {
        fprintf(stderr, "libode_mi355: dmxBatchContactFeedback: n = %lld, but the last tick was given %lld contact joints\n", (long long)n, (long long)b->fb_nc);
        return DMX_EINVAL;
    }
    if (n > 0 && !out) return DMX_EINVAL;
    return feedback_fetch(b, b->fb_nj, n, out);
}

extern "C" int dmxBatchFeedbackDevice(dmxBatchID b, const void **joints_dev, const void **contacts_dev)
{
    if (!b) return DMX_EINVAL;
    { const int rc = dmx_settle(b); if (rc != DMX_OK) return rc; }
    { const int rc = feedback_ready(b, "dmxBatchFeedbackDevice"); if (rc != DMX_OK) return rc; }
    if (joints_dev) *joints_dev = b->fb_devp;
    if (contacts_dev) *contacts_dev = (const char *)b->fb_devp + (size_t)12 * b->fb_nj * b->rsize;
    return DMX_OK;
}

// ---- angular motors (include/dmx_batch.h at DMX_JOINT_AMOTOR) ----------------------------------------------------------------------
// amotor_prepare's records, one per joint of the set, by the activity rules of the tick (dmx_joints.cpp)
void dmx_amotor_records(const dmxBatch *b, dmx::AMotorIn *out)
{
    const int64_t n = b->n;
    auto live = [&](int s) { return s < n && (b->h_bflags[(size_t)s] & dmx::BF_ALIVE) != 0; };
    for (size_t k = 0; k < b->art.size(); k++) {
        const dmxJoint &j = b->art[k];
        dmx::AMotorIn &r = out[k];
        const int s1 = j.body1, s2 = j.body2;
        r.body1 = s1; r.body2 = s2; r.pad = 0;
        r.active = j.kind == DMX_JOINT_AMOTOR && !b->amotor.empty() && !(s1 < 0 && s2 < 0) && s1 != s2 && (s1 < 0 || live(s1)) && (s2 < 0 || live(s2));
        if (r.active) r.m = b->amotor[k];
        else memset(&r.m, 0, sizeof(r.m));
    }
}

static const char *amotor_flaw(const dmxAMotor &m)
{
    auto fin3 = [](const double *p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); };
    if (m.mode != DMX_AMOTOR_USER && m.mode != DMX_AMOTOR_EULER) return "mode is neither DMX_AMOTOR_USER nor DMX_AMOTOR_EULER";
    if (m.num_axes < 1 || m.num_axes > 3) return "num_axes is outside 1..3";
    if (m.mode == DMX_AMOTOR_EULER && m.num_axes != 3) return "Euler mode needs num_axes = 3";
    for (int i = 0; i < 3; i++) {
        if (m.rel[i] < 0 || m.rel[i] > 2) return "rel is outside 0..2";
        if (!fin3(m.axis[i])) return "an axis is not finite";
        if (std::isnan(m.lo_stop[i]) || std::isnan(m.hi_stop[i])) return "a stop is NaN";
    }
    if (!fin3(m.ref1) || !fin3(m.ref2)) return "a reference vector is not finite";
    if (!fin3(m.angle)) return "an angle is not finite";
    if (!fin3(m.vel) || !fin3(m.fmax)) return "vel or fmax is not finite";
    return nullptr;
}

extern "C" int dmxBatchSetAMotors(dmxBatchID b, int64_t n, const dmxAMotor *motors)
{
    if (!b || n < 0 || (n > 0 && !motors)) return DMX_EINVAL;
    if (n != 0 && n != (int64_t)b->art.size()) {
        fprintf(stderr, "libode_mi355: dmxBatchSetAMotors: n = %lld, but the set holds %lld joints\n", (long long)n, (long long)b->art.size());
        return DMX_EINVAL;
    }
    for (int64_t k = 0; k < n; k++) {
        if (b->art[(size_t)k].kind != DMX_JOINT_AMOTOR) continue;        // (only an AMotor's entry is read)
        if (const char *why = amotor_flaw(motors[k])) {
            fprintf(stderr, "libode_mi355: dmxBatchSetAMotors: entry %lld: %s\n", (long long)k, why);
            return DMX_EINVAL;
        }
    }
    { const int rc = dmx_settle(b); if (rc != DMX_OK) return rc; }
    if (n == 0) b->amotor.clear();
    else b->amotor.assign(motors, motors + n);
    return DMX_OK;
}

extern "C" int dmxBatchAMotorFromWorld(dmxBatchID b, int32_t body1, int32_t body2, int mode, int num_axes, const int32_t rel[3],
                                       const double axes_w[3][3], dmxAMotor *out)
{
    if (!b || !out || !axes_w) return DMX_EINVAL;
    if (body1 < -1 || body2 < -1 || body1 >= b->n || body2 >= b->n) return DMX_EINVAL;
    if (mode != DMX_AMOTOR_USER && mode != DMX_AMOTOR_EULER) return DMX_EINVAL;
    if (num_axes < 1 || num_axes > 3 || (mode == DMX_AMOTOR_EULER && num_axes != 3)) return DMX_EINVAL;
    if (mode == DMX_AMOTOR_USER && !rel) return DMX_EINVAL;
    dmxAMotor m;
    memset(&m, 0, sizeof(m));
    m.mode = mode; m.num_axes = num_axes;
    double ax[3][3] = { { 0 } };
    for (int i = 0; i < num_axes; i++) {
        if (mode == DMX_AMOTOR_EULER && i == 1) continue;
        if (mode == DMX_AMOTOR_USER) { if (rel[i] < 0 || rel[i] > 2) return DMX_EINVAL; m.rel[i] = rel[i]; }
        const double *a = axes_w[i];
        const double l = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
        if (!(l > 0) || !std::isfinite(l)) return DMX_EINVAL;
        for (int k = 0; k < 3; k++) ax[i][k] = a[k] / l;
    }
    if (mode == DMX_AMOTOR_EULER) {
        const double d = ax[0][0] * ax[2][0] + ax[0][1] * ax[2][1] + ax[0][2] * ax[2][2];
        if (std::fabs(d) > 1e-9) {
            fprintf(stderr, "libode_mi355: dmxBatchAMotorFromWorld: Euler axes 0 and 2 are not perpendicular (a_0 . a_2 = %g)\n", d);
            return DMX_EINVAL;
        }
        m.rel[0] = 1; m.rel[1] = 0; m.rel[2] = 2;
    }
    // R of the two sides at the current poses (a world side: the identity)
    dmx::M3<double> R[2];
    const int32_t body[2] = { body1, body2 };
    for (int s = 0; s < 2; s++) {
        for (int i = 0; i < 3; i++) for (int k = 0; k < 3; k++) R[s].m[i][k] = i == k ? 1.0 : 0.0;
        if (body[s] < 0) continue;
        double st[13];
        if (b->precision == DMX_F32) {
            float f[13];
            const int rc = dmxBatchDownload(b, DMX_STATE, f, body[s], 1);
            if (rc != DMX_OK) return rc;
            for (int k = 0; k < 13; k++) st[k] = f[k];
        } else {
            const int rc = dmxBatchDownload(b, DMX_STATE, st, body[s], 1);
            if (rc != DMX_OK) return rc;
        }
        const dmx::Q4<double> q = { st[3], st[4], st[5], st[6] };
        R[s] = dmx::quat_to_R(q);
    }
    auto to_frame = [&](int side, const double *w, double *o) {           // R^T w
        const dmx::M3<double> &M = R[side];
        for (int k = 0; k < 3; k++) o[k] = M.m[0][k] * w[0] + M.m[1][k] * w[1] + M.m[2][k] * w[2];
    };
    for (int i = 0; i < num_axes; i++) {
        if (m.rel[i] == 0) for (int k = 0; k < 3; k++) m.axis[i][k] = ax[i][k];
        else to_frame(m.rel[i] - 1, ax[i], m.axis[i]);
    }
    if (mode == DMX_AMOTOR_EULER) { to_frame(0, ax[2], m.ref1); to_frame(1, ax[0], m.ref2); }
    for (int i = 0; i < 3; i++) { m.lo_stop[i] = -__builtin_huge_val(); m.hi_stop[i] = __builtin_huge_val(); }
    *out = m;
    return DMX_OK;
}

extern "C" int dmxBatchAMotorAngles(dmxBatchID b, double *angles3, double *rates3)
{
    if (!b) return DMX_EINVAL;
    { const int rc = dmx_settle(b); if (rc != DMX_OK) return rc; }
    const int64_t nj = (int64_t)b->art.size();
    if (nj == 0) return DMX_OK;
    HIP_TRY(hipSetDevice(b->device));
    { const int rc = dmx_ad_merge(b); if (rc != DMX_OK) return rc; }
    int rc;
    const size_t rs = b->rsize;
    if ((rc = dmx_ensure_dev(b->amotor_in, (size_t)nj * sizeof(dmx::AMotorIn))) != DMX_OK) return rc;
    if ((rc = dmx_ensure_dev(b->amotor_prep, (size_t)(dmx::AMOTOR_PREP_REALS + 3) * nj * rs)) != DMX_OK) return rc;
    b->am_rec.resize((size_t)nj);
    dmx_amotor_records(b, b->am_rec.data());
    // (the records live in pageable host memory: a plain copy, which has read them when it returns)
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemcpy(b->amotor_in.p, b->am_rec.data(), (size_t)nj * sizeof(dmx::AMotorIn), hipMemcpyHostToDevice));
    char *d_prep = (char *)b->amotor_prep.p, *d_rate = d_prep + (size_t)dmx::AMOTOR_PREP_REALS * nj * rs;
    if (b->precision == DMX_F32)
        HIP_TRY(dmx::launch_amotor_prepare<float>((const float *)b->slab, b->stride, (const dmx::AMotorIn *)b->amotor_in.p, (int)nj, 0.0f, (float *)d_prep, (float *)d_rate, b->stream));
    else
        HIP_TRY(dmx::launch_amotor_prepare<double>((const double *)b->slab, b->stride, (const dmx::AMotorIn *)b->amotor_in.p, (int)nj, 0.0, (double *)d_prep, (double *)d_rate, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    // (amotor_prep is the table a tick's prepare pass writes too: every tick with an AMotor row prepares it again in front of its
    //  first kernel, on the same stream, so nothing read it between this call and then)
    std::vector<char> &tmp = b->am_tmp;
    tmp.resize((size_t)(dmx::AMOTOR_PREP_REALS + 3) * nj * rs);
    HIP_TRY(hipMemcpy(tmp.data(), d_prep, tmp.size(), hipMemcpyDeviceToHost));
    auto real_at = [&](size_t i) { return b->precision == DMX_F32 ? (double)((const float *)tmp.data())[i] : ((const double *)tmp.data())[i]; };
    for (int64_t k = 0; k < nj; k++)
        for (int i = 0; i < 3; i++) {
            if (angles3) angles3[3 * k + i] = real_at((size_t)dmx::AMOTOR_PREP_REALS * k + dmx::AMOTOR_AXIS_REALS * i + dmx::AMP_THETA);
            if (rates3) rates3[3 * k + i] = real_at((size_t)dmx::AMOTOR_PREP_REALS * nj + 3 * k + i);
        }
    return DMX_OK;
}

extern "C" int dmxBatchSetJoints(dmxBatchID b, int64_t n, const dmxJoint *joints)
{
    if (!b || n < 0 || (n > 0 && !joints)) return DMX_EINVAL;
    for (int64_t k = 0; k < n; k++)
        if (joints[k].kind < DMX_JOINT_BALL || joints[k].kind > DMX_JOINT_AMOTOR) return DMX_EINVAL;
    { const int rc = dmx_settle(b); if (rc != DMX_OK) return rc; }
    b->art.assign(joints, joints + n);
    b->limot.clear();                    // (they were entries of the old set's joints)
    b->amotor.clear();
    b->fb_valid = false;                 // (so was the last tick's feedback: fb_nj of them, not joint_count())
    return DMX_OK;
}

extern "C" int64_t dmxBatchJointCount(dmxBatchID b) { return b ? (int64_t)b->art.size() : DMX_EINVAL; }

extern "C" int dmxBatchJointFromWorld(dmxBatchID b, int kind, int32_t body1, int32_t body2, const double anchor_w[3], const double axis_w[3],
                                      dmxJoint *out)
{
    const bool needs_axis = kind == DMX_JOINT_HINGE || kind == DMX_JOINT_SLIDER;
    if (!b || !out || !anchor_w || kind < DMX_JOINT_BALL || kind > DMX_JOINT_FIXED || (needs_axis && !axis_w)) return DMX_EINVAL;
    if (body1 < -1 || body2 < -1 || body1 >= b->n || body2 >= b->n) return DMX_EINVAL;
    memset(out, 0, sizeof(*out));
    out->kind = kind; out->body1 = body1; out->body2 = body2;
    double ax[3] = { 0, 0, 0 };
    if (axis_w) {
        const double l = std::sqrt(axis_w[0] * axis_w[0] + axis_w[1] * axis_w[1] + axis_w[2] * axis_w[2]);
        if (needs_axis && !(l > 0)) return DMX_EINVAL;
        if (l > 0) for (int k = 0; k < 3; k++) ax[k] = axis_w[k] / l;
    }
    auto side = [&](int32_t s, double *anchor, double *axis) -> int {
        if (s < 0) { for (int k = 0; k < 3; k++) { anchor[k] = anchor_w[k]; axis[k] = ax[k]; } return DMX_OK; }
        double st[13];
        if (b->precision == DMX_F32) {
            float f[13];
            const int rc = dmxBatchDownload(b, DMX_STATE, f, s, 1);
            if (rc != DMX_OK) return rc;
            for (int k = 0; k < 13; k++) st[k] = f[k];
        } else {
            const int rc = dmxBatchDownload(b, DMX_STATE, st, s, 1);
            if (rc != DMX_OK) return rc;
        }
        const Q4<double> q = { st[3], st[4], st[5], st[6] };
        const M3<double> R = quat_to_R(q);
        const double d[3] = { anchor_w[0] - st[0], anchor_w[1] - st[1], anchor_w[2] - st[2] };
        for (int k = 0; k < 3; k++) {          // R^T
            anchor[k] = R.m[0][k] * d[0] + R.m[1][k] * d[1] + R.m[2][k] * d[2];
            axis[k] = R.m[0][k] * ax[0] + R.m[1][k] * ax[1] + R.m[2][k] * ax[2];
        }
        return DMX_OK;
    };
    int rc = side(body1, out->anchor1, out->axis1);
    if (rc == DMX_OK) rc = side(body2, out->anchor2, out->axis2);
    return rc;
}

extern "C" int dmxBatchJointErrors(dmxBatchID b, double *pos_err, double *axis_err, double out_max[2])
{
    if (!b) return DMX_EINVAL;
    { const int rc = dmx_settle(b); if (rc != DMX_OK) return rc; }
    if (out_max) out_max[0] = out_max[1] = 0.0;
    const int64_t nj = (int64_t)b->art.size();
    if (nj == 0) return DMX_OK;
    HIP_TRY(hipSetDevice(b->device));
    int rc;
    if ((rc = dmx_ensure_dev(b->art_dev, (size_t)nj * sizeof(dmxJoint))) != DMX_OK) return rc;
    if ((rc = dmx_ensure_dev(b->art_err, ((size_t)2 * nj + 2) * sizeof(double))) != DMX_OK) return rc;
    // (the zero poses are read for sliders and fixed joints only: a set without them copies what it always did)
    bool lim = false;
    if (!b->limot.empty()) for (const dmxJoint &j : b->art) lim = lim || j.kind == DMX_JOINT_SLIDER || j.kind == DMX_JOINT_FIXED;
    if (lim && (rc = dmx_ensure_dev(b->limot_dev, (size_t)nj * sizeof(dmxHingeLimot))) != DMX_OK) return rc;
    double *d_pos = (double *)b->art_err.p + 2, *d_axis = d_pos + nj;
    unsigned long long *d_max = (unsigned long long *)b->art_err.p;
    // (the set lives in pageable host memory: plain copies, which have read it when they return)
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemcpy(b->art_dev.p, b->art.data(), (size_t)nj * sizeof(dmxJoint), hipMemcpyHostToDevice));
    if (lim) HIP_TRY(hipMemcpy(b->limot_dev.p, b->limot.data(), (size_t)nj * sizeof(dmxHingeLimot), hipMemcpyHostToDevice));
    const dmxHingeLimot *d_lim = lim ? (const dmxHingeLimot *)b->limot_dev.p : nullptr;
    HIP_TRY(hipMemsetAsync(d_max, 0, 2 * sizeof(double), b->stream));
    const unsigned grid = (unsigned)((nj + 255) / 256);
    if (b->precision == DMX_F32)
        hipLaunchKernelGGL((dmx::joint_errors<float>), dim3(grid), dim3(256), 0, b->stream, (const float *)b->slab, b->bflags, b->stride, b->n,
                           (const dmxJoint *)b->art_dev.p, d_lim, nj, d_pos, d_axis, d_max);
    else
        hipLaunchKernelGGL((dmx::joint_errors<double>), dim3(grid), dim3(256), 0, b->stream, (const double *)b->slab, b->bflags, b->stride, b->n,
                           (const dmxJoint *)b->art_dev.p, d_lim, nj, d_pos, d_axis, d_max);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (pos_err) HIP_TRY(hipMemcpy(pos_err, d_pos, (size_t)nj * sizeof(double), hipMemcpyDeviceToHost));
    if (axis_err) HIP_TRY(hipMemcpy(axis_err, d_axis, (size_t)nj * sizeof(double), hipMemcpyDeviceToHost));
    if (out_max) HIP_TRY(hipMemcpy(out_max, d_max, 2 * sizeof(double), hipMemcpyDeviceToHost));
    return DMX_OK;
}

extern "C" int dmxBatchSetHingeLimots(dmxBatchID b, int64_t n, const dmxHingeLimot *limots)
{
    if (!b || n < 0 || (n > 0 && !limots)) return DMX_EINVAL;
    if (n != 0 && n != (int64_t)b->art.size()) return DMX_EINVAL;
    for (int64_t k = 0; k < n; k++) {
        const dmxHingeLimot &l = limots[k];
        if (!std::isfinite(l.vel) || !std::isfinite(l.fmax) || std::isnan(l.lo_stop) || std::isnan(l.hi_stop)) return DMX_EINVAL;
    }
    { const int rc = dmx_settle(b); if (rc != DMX_OK) return rc; }
    if (n == 0) b->limot.clear();
    else b->limot.assign(limots, limots + n);
    return DMX_OK;
}

extern "C" int dmxBatchHingeLimotInit(dmxBatchID b, const dmxJoint *joint, dmxHingeLimot *out)
{
    if (!b || !joint || !out) return DMX_EINVAL;
    if (joint->body1 < -1 || joint->body2 < -1 || joint->body1 >= b->n || joint->body2 >= b->n) return DMX_EINVAL;
    auto quat = [&](int32_t s, dmx::Q4<double> &q) -> int {
        q = { 1.0, 0.0, 0.0, 0.0 };
        if (s < 0) return DMX_OK;
        double st[13];
        if (b->precision == DMX_F32) {
            float f[13];
            const int rc = dmxBatchDownload(b, DMX_STATE, f, s, 1);
            if (rc != DMX_OK) return rc;
            for (int k = 0; k < 13; k++) st[k] = f[k];
        } else {
            const int rc = dmxBatchDownload(b, DMX_STATE, st, s, 1);
            if (rc != DMX_OK) return rc;
        }
        q = { st[3], st[4], st[5], st[6] };
        return DMX_OK;
    };
    dmx::Q4<double> q1, q2;
    int rc = quat(joint->body1, q1);
    if (rc == DMX_OK) rc = quat(joint->body2, q2);
    if (rc != DMX_OK) return rc;
    const dmx::Q4<double> r = dmx::qmul(dmx::qconj(q1), q2);
    out->lo_stop = -__builtin_huge_val(); out->hi_stop = __builtin_huge_val(); out->vel = 0.0; out->fmax = 0.0;
    out->qrel0[0] = r.w; out->qrel0[1] = r.x; out->qrel0[2] = r.y; out->qrel0[3] = r.z;
    return DMX_OK;
}

extern "C" int dmxBatchHingeAngles(dmxBatchID b, double *angle, double *rate)
{
    if (!b) return DMX_EINVAL;
    { const int rc = dmx_settle(b); if (rc != DMX_OK) return rc; }
    const int64_t nj = (int64_t)b->art.size();
    if (nj == 0) return DMX_OK;
    HIP_TRY(hipSetDevice(b->device));
    int rc;
    const bool lim = !b->limot.empty();
    if ((rc = dmx_ensure_dev(b->art_dev, (size_t)nj * sizeof(dmxJoint))) != DMX_OK) return rc;
    if ((rc = dmx_ensure_dev(b->art_err, ((size_t)2 * nj + 2) * sizeof(double))) != DMX_OK) return rc;
    if (lim && (rc = dmx_ensure_dev(b->limot_dev, (size_t)nj * sizeof(dmxHingeLimot))) != DMX_OK) return rc;
    double *d_angle = (double *)b->art_err.p + 2, *d_rate = d_angle + nj;
    // (the sets live in pageable host memory: plain copies, which have read them when they return)
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemcpy(b->art_dev.p, b->art.data(), (size_t)nj * sizeof(dmxJoint), hipMemcpyHostToDevice));
    if (lim) HIP_TRY(hipMemcpy(b->limot_dev.p, b->limot.data(), (size_t)nj * sizeof(dmxHingeLimot), hipMemcpyHostToDevice));
    const dmxHingeLimot *d_lim = lim ? (const dmxHingeLimot *)b->limot_dev.p : nullptr;
    const unsigned grid = (unsigned)((nj + 255) / 256);
    if (b->precision == DMX_F32)
        hipLaunchKernelGGL((dmx::hinge_angles<float>), dim3(grid), dim3(256), 0, b->stream, (const float *)b->slab, b->bflags, b->stride, b->n,
                           (const dmxJoint *)b->art_dev.p, d_lim, nj, d_angle, d_rate);
    else
        hipLaunchKernelGGL((dmx::hinge_angles<double>), dim3(grid), dim3(256), 0, b->stream, (const double *)b->slab, b->bflags, b->stride, b->n,
                           (const dmxJoint *)b->art_dev.p, d_lim, nj, d_angle, d_rate);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (angle) HIP_TRY(hipMemcpy(angle, d_angle, (size_t)nj * sizeof(double), hipMemcpyDeviceToHost));
    if (rate) HIP_TRY(hipMemcpy(rate, d_rate, (size_t)nj * sizeof(double), hipMemcpyDeviceToHost));
    return DMX_OK;
}

extern "C" int dmxBatchSliderPositions(dmxBatchID b, double *pos, double *rate)
{
    if (!b) return DMX_EINVAL;
    { const int rc = dmx_settle(b); if (rc != DMX_OK) return rc; }
    const int64_t nj = (int64_t)b->art.size();
    if (nj == 0) return DMX_OK;
    HIP_TRY(hipSetDevice(b->device));
    int rc;
    if ((rc = dmx_ensure_dev(b->art_dev, (size_t)nj * sizeof(dmxJoint))) != DMX_OK) return rc;
    if ((rc = dmx_ensure_dev(b->art_err, ((size_t)2 * nj + 2) * sizeof(double))) != DMX_OK) return rc;
    double *d_pos = (double *)b->art_err.p + 2, *d_rate = d_pos + nj;
    // (the set lives in pageable host memory: a plain copy, which has read it when it returns)
    HIP_TRY(hipStreamSynchronize(b->stream));
    HIP_TRY(hipMemcpy(b->art_dev.p, b->art.data(), (size_t)nj * sizeof(dmxJoint), hipMemcpyHostToDevice));
    const unsigned grid = (unsigned)((nj + 255) / 256);
    if (b->precision == DMX_F32)
        hipLaunchKernelGGL((dmx::slider_positions<float>), dim3(grid), dim3(256), 0, b->stream, (const float *)b->slab, b->bflags, b->stride, b->n,
                           (const dmxJoint *)b->art_dev.p, nj, d_pos, d_rate);
    else
        hipLaunchKernelGGL((dmx::slider_positions<double>), dim3(grid), dim3(256), 0, b->stream, (const double *)b->slab, b->bflags, b->stride, b->n,
                           (const dmxJoint *)b->art_dev.p, nj, d_pos, d_rate);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (pos) HIP_TRY(hipMemcpy(pos, d_pos, (size_t)nj * sizeof(double), hipMemcpyDeviceToHost));
    if (rate) HIP_TRY(hipMemcpy(rate, d_rate, (size_t)nj * sizeof(double), hipMemcpyDeviceToHost));
    return DMX_OK;
}
