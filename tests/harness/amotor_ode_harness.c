/*
 * amotor_ode_harness.c -- a two-link arm on ball joints with an Euler angular motor beside each, through include/ode/ode.h alone, and
 * the same arm through include/dmx_batch.h: a plain C99 client of both headers, built once per width of dReal (-DdDOUBLE against
 * libode_mi355, -DdSINGLE against libode_mi355_single), for tests/test_gpu_amotor_ode.py.
 *
 *   amotor_ode_harness ode|batch|torque_joint|torque_body step|quick
 * world - ball A + AMotor A - link 1 - ball B + AMotor B - link 2.  AMotor A is attached as (0, link 1) -- the exchange of sides --,
 * AMotor B as (link 2, link 1).  Joints and motors are made with the links unrotated (axis 0 = +x with the first side, axis 2 = +z
 * with the second: that pose is angles zero), then the links are posed: link 1 so that AMotor A stands at the angles TA, link 2 so
 * that AMotor B stands at TB.  TB's middle angle, 0.6, lies beyond AMotor B's stop dParamHiStop2 = 0.3.
 * ode           prints "ANG k e0 e1 e2 g0 g1 g2" per AMotor (the angles posed, dJointGetAMotorAngle's), "PAR ..." (the getters' echo),
 *               then per tick "S" + 26 numbers (%.17g: pos3 quat4 lvel3 avel3 of both links) and "TH" + AMotor B's three angles
 * batch         the twin: the same uploads and the same joints through the batch interface; prints the "S" lines
 * torque_joint  as ode, with dJointAddAMotorTorques(AMotor B, T1, T2, T3) before every tick
 * torque_body   as ode, with dBodyAddTorque of +-sum T_i a_i (dJointGetAMotorAxis) on link 2 / link 1 instead
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include "dmx_batch.h"
#include "ode/ode.h"

#define TICKS 40
#define CAPACITY 512            /* dWorldCreate's first batch */
#define H ((dReal)(1.0 / 60.0))
#define MUST(call) do { int rc_ = (call); if (rc_ != DMX_OK) { printf("FAIL %s -> %d\n", #call, rc_); return 1; } } while (0)

static const double TA[3] = { 0.25, -0.4, 0.3 }, TB[3] = { -0.2, 0.6, 0.35 };
static const dReal T1 = (dReal)0.3, T2 = (dReal)-0.2, T3 = (dReal)0.1;
enum { ODE, BATCH, TORQUE_JOINT, TORQUE_BODY };

static void qmul(const double a[4], const double b[4], double o[4])
{
    o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    o[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
    o[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}
static void axis_angle(int axis, double angle, double q[4])
{
    q[0] = cos(0.5 * angle); q[1] = q[2] = q[3] = 0;
    q[1 + axis] = sin(0.5 * angle);
}
/* D = Rot(z, t2) Rot(y, t1) Rot(x, t0): a_0 = x, a_2 = z, a_1 = a_2 x a_0 = y */
static void compose(const double t[3], double d[4])
{
    double qx[4], qy[4], qz[4], tmp[4];
    axis_angle(0, t[0], qx); axis_angle(1, t[1], qy); axis_angle(2, t[2], qz);
    qmul(qy, qx, tmp); qmul(qz, tmp, d);
}
static void rotate(const double q[4], const double v[3], double o[3])
{
    const double p[4] = { 0, v[0], v[1], v[2] }, c[4] = { q[0], -q[1], -q[2], -q[3] };
    double t[4], r[4];
    qmul(q, p, t); qmul(t, c, r);
    o[0] = r[1]; o[1] = r[2]; o[2] = r[3];
}
/* the posed arm: quaternions and positions of the two links, as dReal */
static void pose(dReal q1[4], dReal x1[3], dReal q2[4], dReal x2[3])
{
    double da[4], db[4], qa[4], qb[4], up[3] = { 0, 0.5, 0 }, down[3] = { 0, -0.5, 0 }, v[3], anchor_b[3];
    int k;
    compose(TA, da); compose(TB, db);
    qa[0] = da[0]; qa[1] = -da[1]; qa[2] = -da[2]; qa[3] = -da[3];      /* side 1 of AMotor A is the world: link 1 turns the other way */
    qmul(qa, db, qb);                                                   /* link 2 at D_B against link 1: a turn common to both changes no angle */
    rotate(qa, down, v);
    for (k = 0; k < 3; k++) { x1[k] = (dReal)v[k]; anchor_b[k] = 2 * v[k]; }
    rotate(qb, up, v);
    for (k = 0; k < 3; k++) x2[k] = (dReal)(anchor_b[k] - v[k]);
    for (k = 0; k < 4; k++) { q1[k] = (dReal)qa[k]; q2[k] = (dReal)qb[k]; }
}
static const dReal LV[2][3] = { { 0.1f, 0.0f, -0.2f }, { -0.3f, 0.2f, 0.1f } }, AV[2][3] = { { 0.2f, -0.1f, 0.3f }, { -0.4f, 0.5f, 0.2f } };

static void print_state(const double *s, int n)
{
    int k;
    printf("S");
    for (k = 0; k < n; k++) printf(" %.17g", s[k]);
    printf("\n");
}

static int run_ode(int mode, int quick)
{
    dWorldID w;
    dBodyID b[2];
    dJointID ball_a, ball_b, am[2];
    dReal q1[4], x1[3], q2[4], x2[3];
    int i, k, t;
    dInitODE();
    w = dWorldCreate();
    dWorldSetGravity(w, 0, (dReal)-9.8, 0);
    dWorldSetCFM(w, (dReal)1e-5);
    b[0] = dBodyCreate(w); b[1] = dBodyCreate(w);
    dBodySetPosition(b[0], 0, (dReal)-0.5, 0);
    dBodySetPosition(b[1], 0, (dReal)-1.5, 0);
    ball_a = dJointCreateBall(w, 0); dJointAttach(ball_a, b[0], 0); dJointSetBallAnchor(ball_a, 0, 0, 0);
    ball_b = dJointCreateBall(w, 0); dJointAttach(ball_b, b[1], b[0]); dJointSetBallAnchor(ball_b, 0, -1, 0);
    am[0] = dJointCreateAMotor(w, 0); dJointAttach(am[0], 0, b[0]);
    am[1] = dJointCreateAMotor(w, 0); dJointAttach(am[1], b[1], b[0]);
    for (i = 0; i < 2; i++) {
        dJointSetAMotorMode(am[i], dAMotorEuler);
        dJointSetAMotorAxis(am[i], 0, 1, 1, 0, 0);
        dJointSetAMotorAxis(am[i], 2, 2, 0, 0, 1);
    }
    /* A: a motor on axis 0, stops on the others; B: stops everywhere, the middle one violated */
    dJointSetAMotorParam(am[0], dParamVel, (dReal)0.5); dJointSetAMotorParam(am[0], dParamFMax, 2);
    dJointSetAMotorParam(am[0], dParamLoStop2, -1); dJointSetAMotorParam(am[0], dParamHiStop2, 1);
    dJointSetAMotorParam(am[0], dParamLoStop3, -1); dJointSetAMotorParam(am[0], dParamHiStop3, 1);
    dJointSetAMotorParam(am[1], dParamLoStop, -1); dJointSetAMotorParam(am[1], dParamHiStop, 1);
    dJointSetAMotorParam(am[1], dParamLoStop2, (dReal)-0.3); dJointSetAMotorParam(am[1], dParamHiStop2, (dReal)0.3);
    dJointSetAMotorParam(am[1], dParamLoStop3, -1); dJointSetAMotorParam(am[1], dParamHiStop3, 1);
    pose(q1, x1, q2, x2);
    dBodySetQuaternion(b[0], q1); dBodySetPosition(b[0], x1[0], x1[1], x1[2]);
    dBodySetQuaternion(b[1], q2); dBodySetPosition(b[1], x2[0], x2[1], x2[2]);
    for (i = 0; i < 2; i++) { dBodySetLinearVel(b[i], LV[i][0], LV[i][1], LV[i][2]); dBodySetAngularVel(b[i], AV[i][0], AV[i][1], AV[i][2]); }
    if (mode == ODE) {
        for (i = 0; i < 2; i++) {
            const double *e = i ? TB : TA;
            printf("ANG %d %.17g %.17g %.17g %.17g %.17g %.17g\n", i, e[0], e[1], e[2], (double)dJointGetAMotorAngle(am[i], 0),
                   (double)dJointGetAMotorAngle(am[i], 1), (double)dJointGetAMotorAngle(am[i], 2));
        }
        printf("PAR %d %d %d %d %d %d %.17g %.17g %.17g %.17g %d %d\n", dJointGetType(am[0]), dJointGetAMotorMode(am[0]), dJointGetAMotorNumAxes(am[0]),
               dJointGetAMotorAxisRel(am[0], 0), dJointGetAMotorAxisRel(am[0], 2), dJointGetBody(am[0], 0) == b[0],
               (double)dJointGetAMotorParam(am[1], dParamHiStop2), (double)dJointGetAMotorParam(am[0], dParamFMax),
               (double)dJointGetAMotorParam(am[0], dParamLoStop3), (double)dJointGetAMotorParam(am[1], dParamLoStop),
               dAreConnected(b[0], b[1]), dJointGetBody(am[0], 1) == 0);
    }
    for (t = 0; t < TICKS; t++) {
        double s[26];
        if (mode == TORQUE_JOINT) dJointAddAMotorTorques(am[1], T1, T2, T3);
        if (mode == TORQUE_BODY) {
            const dReal tq[3] = { T1, T2, T3 };
            double sum[3] = { 0, 0, 0 };
            for (i = 0; i < 3; i++) {
                dVector3 a;
                dJointGetAMotorAxis(am[1], i, a);
                for (k = 0; k < 3; k++) sum[k] += (double)tq[i] * (double)a[k];
            }
            dBodyAddTorque(b[1], (dReal)sum[0], (dReal)sum[1], (dReal)sum[2]);
            dBodyAddTorque(b[0], (dReal)-sum[0], (dReal)-sum[1], (dReal)-sum[2]);
        }
        if ((quick ? dWorldQuickStep(w, H) : dWorldStep(w, H)) != 1) { printf("FAIL step\n"); return 1; }
        for (i = 0; i < 2; i++) {
            const dReal *p = dBodyGetPosition(b[i]), *q = dBodyGetQuaternion(b[i]), *v = dBodyGetLinearVel(b[i]), *a = dBodyGetAngularVel(b[i]);
            for (k = 0; k < 3; k++) { s[13 * i + k] = p[k]; s[13 * i + 7 + k] = v[k]; s[13 * i + 10 + k] = a[k]; }
            for (k = 0; k < 4; k++) s[13 * i + 3 + k] = q[k];
        }
        print_state(s, 26);
        printf("TH %.17g %.17g %.17g %.17g\n", (double)dJointGetAMotorAngle(am[1], 0), (double)dJointGetAMotorAngle(am[1], 1),
               (double)dJointGetAMotorAngle(am[1], 2), (double)dJointGetAMotorAngleRate(am[1], 1));
    }
    dWorldDestroy(w);
    dCloseODE();
    return 0;
}

static int run_batch(int quick)
{
    static dReal state[CAPACITY * 13], one[CAPACITY], three[CAPACITY * 3], zero[CAPACITY * 3];
    static uint8_t flags[CAPACITY];
    static const double axes[3][3] = { { 1, 0, 0 }, { 0, 0, 0 }, { 0, 0, 1 } }, origin[3] = { 0, 0, 0 }, anchor_b[3] = { 0, -1, 0 };
    dmxBatchID b;
    dmxJoint joints[4];
    dmxAMotor motors[4];
    dReal q1[4], x1[3], q2[4], x2[3];
    int i, k, t;
    /* the quaternions as dBodySetQuaternion keeps them */
    {
        dWorldID w0;
        dBodyID b0;
        dInitODE();
        w0 = dWorldCreate();
        b0 = dBodyCreate(w0);
        pose(q1, x1, q2, x2);
        dBodySetQuaternion(b0, q1); memcpy(q1, dBodyGetQuaternion(b0), sizeof q1);
        dBodySetQuaternion(b0, q2); memcpy(q2, dBodyGetQuaternion(b0), sizeof q2);
        dWorldDestroy(w0);
    }
    MUST(dmxBatchCreate(&b, CAPACITY, sizeof(dReal) == 4 ? DMX_F32 : DMX_F64, 0));
    for (i = 0; i < CAPACITY; i++) {
        for (k = 0; k < 13; k++) state[i * 13 + k] = (dReal)(k == 3);          /* an empty slot: unit quaternion, unit mass */
        one[i] = 1; three[3 * i] = three[3 * i + 1] = three[3 * i + 2] = 1;
        flags[i] = 0;
    }
    state[1] = (dReal)-0.5; state[13 + 1] = (dReal)-1.5;
    flags[0] = flags[1] = DMX_BODY_ALIVE;
    MUST(dmxBatchUpload(b, DMX_STATE, state, 0, CAPACITY));
    MUST(dmxBatchUpload(b, DMX_MASS, one, 0, CAPACITY));
    MUST(dmxBatchUpload(b, DMX_INERTIA, three, 0, CAPACITY));
    MUST(dmxBatchUpload(b, DMX_FORCE, zero, 0, CAPACITY));
    MUST(dmxBatchUpload(b, DMX_TORQUE, zero, 0, CAPACITY));
    MUST(dmxBatchUploadBodyFlags(b, flags, 0, CAPACITY));
    MUST(dmxBatchSetGravity(b, 0, (dReal)-9.8, 0));
    MUST(dmxBatchSetERP(b, (dReal)0.2));
    MUST(dmxBatchSetCFM(b, (dReal)1e-5));
    MUST(dmxBatchSetQuickStep(b, 20, (dReal)1.3));
    MUST(dmxBatchSetStepper(b, quick ? DMX_STEPPER_QUICK : DMX_STEPPER_EXACT));
    /* the joints and the motors at the unrotated pose */
    MUST(dmxBatchJointFromWorld(b, DMX_JOINT_BALL, 0, -1, origin, NULL, &joints[0]));
    MUST(dmxBatchJointFromWorld(b, DMX_JOINT_BALL, 1, 0, anchor_b, NULL, &joints[1]));
    memset(&joints[2], 0, 2 * sizeof joints[0]);
    joints[2].kind = DMX_JOINT_AMOTOR; joints[2].body1 = -1; joints[2].body2 = 0;
    joints[3].kind = DMX_JOINT_AMOTOR; joints[3].body1 = 1; joints[3].body2 = 0;
    memset(motors, 0, sizeof motors);
    for (i = 0; i < 2; i++) {
        motors[i].num_axes = 1;
        for (k = 0; k < 3; k++) { motors[i].lo_stop[k] = -(double)dInfinity; motors[i].hi_stop[k] = (double)dInfinity; }
    }
    MUST(dmxBatchAMotorFromWorld(b, -1, 0, DMX_AMOTOR_EULER, 3, NULL, axes, &motors[2]));
    MUST(dmxBatchAMotorFromWorld(b, 1, 0, DMX_AMOTOR_EULER, 3, NULL, axes, &motors[3]));
    motors[2].vel[0] = (dReal)0.5; motors[2].fmax[0] = 2;
    motors[2].lo_stop[1] = motors[2].lo_stop[2] = -1; motors[2].hi_stop[1] = motors[2].hi_stop[2] = 1;
    motors[3].lo_stop[0] = motors[3].lo_stop[2] = -1; motors[3].hi_stop[0] = motors[3].hi_stop[2] = 1;
    motors[3].lo_stop[1] = (dReal)-0.3; motors[3].hi_stop[1] = (dReal)0.3;
    MUST(dmxBatchSetJoints(b, 4, joints));
    MUST(dmxBatchSetAMotors(b, 4, motors));
    /* the posed arm */
    for (k = 0; k < 3; k++) { state[k] = x1[k]; state[13 + k] = x2[k]; state[7 + k] = LV[0][k]; state[13 + 7 + k] = LV[1][k]; state[10 + k] = AV[0][k]; state[13 + 10 + k] = AV[1][k]; }
    for (k = 0; k < 4; k++) { state[3 + k] = q1[k]; state[13 + 3 + k] = q2[k]; }
    MUST(dmxBatchUpload(b, DMX_STATE, state, 0, 2));
    for (t = 0; t < TICKS; t++) {
        double s[26];
        MUST(dmxBatchStepJoints(b, H, 0, NULL));
        MUST(dmxBatchDownload(b, DMX_STATE, state, 0, 2));
        for (k = 0; k < 26; k++) s[k] = state[k];
        print_state(s, 26);
    }
    MUST(dmxBatchDestroy(b));
    dCloseODE();
    return 0;
}

int main(int argc, char **argv)
{
    int mode, quick;
    if (argc != 3) { fprintf(stderr, "usage: amotor_ode_harness ode|batch|torque_joint|torque_body step|quick\n"); return 2; }
    mode = !strcmp(argv[1], "ode") ? ODE : !strcmp(argv[1], "batch") ? BATCH : !strcmp(argv[1], "torque_joint") ? TORQUE_JOINT :
           !strcmp(argv[1], "torque_body") ? TORQUE_BODY : -1;
    quick = !strcmp(argv[2], "quick");
    if (mode < 0 || (!quick && strcmp(argv[2], "step"))) { fprintf(stderr, "bad arguments\n"); return 2; }
    return mode == BATCH ? run_batch(quick) : run_ode(mode, quick);
}
