/*
 * stability_tick_harness.c -- damping, the maximum angular speed and the contact correction scalars through include/ode/ode.h, and
 * the same scene through include/dmx_batch.h: a plain C99 client of both headers, built once per width of dReal (-DdDOUBLE against
 * libode_mi355, -DdSINGLE against libode_mi355_single), for tests/test_gpu_stability_ode.py.
 *
 *   stability_tick_harness ode|batch step|quick [plain|grow]
 * ode    dWorldSetDamping & co. before most bodies are made, per-body overrides, dWorldSetContactSurfaceLayer / MaxCorrectingVel, then
 *        TICKS ticks of dWorldStep or dWorldQuickStep with explicit contact joints.  Checks on the way that every getter returns what
 *        was set, that a body made after dWorldSetDamping inherits the world's values and an earlier one does not, and that values
 *        out of range are ignored; any miss is a line "FAIL ..." and exit status 1.
 * batch  the twin: a batch of the ODE world's first capacity, the same uploads dWorldStep makes, the same table and scalars through
 *        dmxBatchUploadBodyDamping / dmxBatchSetContactCorrection, the same ticks through dmxBatchStepJoints.
 * plain  (either mode) no knob is touched at all.
 * grow   (either mode) after GROW_AT ticks NF more bodies are made, which the world's first batch cannot hold: the ODE world moves to
 *        a batch of twice the capacity and must carry the table and the two scalars over; the twin has that capacity from the start
 *        and brings the new slots to life then.  The new bodies inherit the world's values; the first and the last are printed too.
 * Both print, per tick and body, 13 numbers (%.17g): pos3 quat4 lvel3 avel3.  The test compares the two outputs as text.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include "dmx_batch.h"
#include "ode/ode.h"

#define NB 6
#define NC 6
#define TICKS 6
#define CAPACITY 512            /* dWorldCreate's first batch */
#define NF 520                  /* grow: more bodies than that batch holds */
#define GROW_AT 3
#define MAXCAP (2 * CAPACITY)
#define H ((dReal)(1.0 / 60.0))

static int failures = 0, grow = 0;
#define EXPECT(cond) do { if (!(cond)) { printf("FAIL %s (line %d)\n", #cond, __LINE__); failures++; } } while (0)
#define MUST(call) do { int rc_ = (call); if (rc_ != DMX_OK) { printf("FAIL %s -> %d\n", #call, rc_); return 1; } } while (0)

/* the scene: bodies 0..3 rest on static ground with one or two contacts each, 4 spins freely, 5 is kinematic */
static const dReal POS[NB][3] = { { 0, 0.5f, 0 }, { 3, 0.5f, 0 }, { 6, 0.5f, 0 }, { 9, 0.5f, 0 }, { 12, 3, 0 }, { 15, 3, 0 } };
static const dReal LVEL[NB][3] = { { 0.2f, -1.0f, 0.1f }, { 0, -0.5f, 0 }, { 0.4f, -0.25f, 0 }, { 0.015f, 0, 0 }, { 0.5f, 0.25f, 0 }, { 1, 0.5f, 0.25f } };
static const dReal AVEL[NB][3] = { { 0.5f, 0, 0.25f }, { 0, 2, 0 }, { 0.125f, 0, 0 }, { 0, 0.005f, 0 }, { 1.5f, -2, 0.75f }, { 3, 1, -2 } };
static const struct { int body; dReal off[3], depth; int bounce; } CON[NC] = {
    { 0, { 0.25f, -0.5f, 0 }, 0.005f, 1 }, { 0, { -0.25f, -0.5f, 0.125f }, 0.03125f, 0 }, { 1, { 0, -0.5f, 0 }, 0.0625f, 0 },
    { 2, { 0.125f, -0.5f, 0 }, 0.0234375f, 0 }, { 2, { -0.125f, -0.5f, 0.25f }, 0.015625f, 0 }, { 3, { 0, -0.5f, 0 }, 0.046875f, 0 },
};
#define LAYER ((dReal)0.02)
#define VMAX ((dReal)0.15)
/* the table the ODE calls below come to, per body: lin_scale ang_scale lin_threshold ang_threshold max_angular_speed */
static dmxBodyDamping expected[NB];

static void print_state(const double s[13])
{
    int k;
    for (k = 0; k < 13; k++) printf("%.17g%c", s[k], k == 12 ? '\n' : ' ');
}

static int run_ode(int quick, int plain)
{
    dWorldID w;
    dJointGroupID group;
    static dBodyID b[NB + NF];
    int i, k, t, nb = NB;
    dInitODE();
    w = dWorldCreate();
    group = dJointGroupCreate(0);
    dWorldSetGravity(w, 0, (dReal)-9.8, 0);
    dWorldSetCFM(w, (dReal)1e-5);
    /* the defaults */
    EXPECT(dWorldGetLinearDamping(w) == 0 && dWorldGetAngularDamping(w) == 0);
    EXPECT(dWorldGetLinearDampingThreshold(w) == (dReal)0.01 && dWorldGetAngularDampingThreshold(w) == (dReal)0.01);
    EXPECT(dWorldGetMaxAngularSpeed(w) == dInfinity);
    EXPECT(dWorldGetContactSurfaceLayer(w) == 0 && dWorldGetContactMaxCorrectingVel(w) == dInfinity);
    b[0] = dBodyCreate(w);                      /* made before the world's values change: keeps the defaults */
    if (!plain) {
        dWorldSetDamping(w, (dReal)0.0625, (dReal)0.125);
        dWorldSetLinearDampingThreshold(w, (dReal)0.25);
        dWorldSetAngularDampingThreshold(w, (dReal)0.375);
        dWorldSetMaxAngularSpeed(w, (dReal)1.5);
        dWorldSetContactSurfaceLayer(w, LAYER);
        dWorldSetContactMaxCorrectingVel(w, VMAX);
        EXPECT(dWorldGetLinearDamping(w) == (dReal)0.0625 && dWorldGetAngularDamping(w) == (dReal)0.125);
        EXPECT(dWorldGetLinearDampingThreshold(w) == (dReal)0.25 && dWorldGetAngularDampingThreshold(w) == (dReal)0.375);
        EXPECT(dWorldGetMaxAngularSpeed(w) == (dReal)1.5);
        EXPECT(dWorldGetContactSurfaceLayer(w) == LAYER && dWorldGetContactMaxCorrectingVel(w) == VMAX);
        /* out of range: ignored (one line on stderr each) */
        dWorldSetLinearDamping(w, (dReal)1.5); dWorldSetAngularDamping(w, (dReal)-0.5); dWorldSetLinearDampingThreshold(w, (dReal)-1);
        dWorldSetMaxAngularSpeed(w, 0); dWorldSetContactSurfaceLayer(w, (dReal)-0.001); dWorldSetContactMaxCorrectingVel(w, 0);
        EXPECT(dWorldGetLinearDamping(w) == (dReal)0.0625 && dWorldGetAngularDamping(w) == (dReal)0.125 && dWorldGetLinearDampingThreshold(w) == (dReal)0.25);
        EXPECT(dWorldGetMaxAngularSpeed(w) == (dReal)1.5 && dWorldGetContactSurfaceLayer(w) == LAYER && dWorldGetContactMaxCorrectingVel(w) == VMAX);
    }
    for (i = 1; i < NB; i++) b[i] = dBodyCreate(w);
    if (!plain) {
        EXPECT(dBodyGetLinearDamping(b[0]) == 0 && dBodyGetAngularDamping(b[0]) == 0 && dBodyGetMaxAngularSpeed(b[0]) == dInfinity);
        EXPECT(dBodyGetLinearDampingThreshold(b[0]) == (dReal)0.01 && dBodyGetAngularDampingThreshold(b[0]) == (dReal)0.01);
        for (i = 1; i < NB; i++) {
            EXPECT(dBodyGetLinearDamping(b[i]) == (dReal)0.0625 && dBodyGetAngularDamping(b[i]) == (dReal)0.125);
            EXPECT(dBodyGetLinearDampingThreshold(b[i]) == (dReal)0.25 && dBodyGetAngularDampingThreshold(b[i]) == (dReal)0.375);
            EXPECT(dBodyGetMaxAngularSpeed(b[i]) == (dReal)1.5);
        }
        /* per-body overrides */
        dBodySetDamping(b[1], (dReal)0.5, 0);
        dBodySetLinearDampingThreshold(b[1], (dReal)0.125);
        dBodySetAngularDampingThreshold(b[2], (dReal)0.0625);
        dBodySetMaxAngularSpeed(b[2], dInfinity);
        dBodySetMaxAngularSpeed(b[4], (dReal)0.75);
        dBodySetLinearDamping(b[3], (dReal)2);             /* ignored */
        dBodySetDampingDefaults(b[0]);                     /* now the world's */
        dBodySetAngularDamping(b[0], (dReal)0.25);
        EXPECT(dBodyGetLinearDamping(b[1]) == (dReal)0.5 && dBodyGetAngularDamping(b[1]) == 0 && dBodyGetLinearDampingThreshold(b[1]) == (dReal)0.125);
        EXPECT(dBodyGetAngularDampingThreshold(b[2]) == (dReal)0.0625 && dBodyGetMaxAngularSpeed(b[2]) == dInfinity);
        EXPECT(dBodyGetMaxAngularSpeed(b[4]) == (dReal)0.75 && dBodyGetLinearDamping(b[3]) == (dReal)0.0625);
        EXPECT(dBodyGetLinearDamping(b[0]) == (dReal)0.0625 && dBodyGetAngularDamping(b[0]) == (dReal)0.25 && dBodyGetMaxAngularSpeed(b[0]) == (dReal)1.5);
        for (i = 0; i < NB; i++) {
            EXPECT(dBodyGetLinearDamping(b[i]) == (dReal)expected[i].lin_scale && dBodyGetAngularDamping(b[i]) == (dReal)expected[i].ang_scale);
            EXPECT(dBodyGetLinearDampingThreshold(b[i]) == (dReal)expected[i].lin_threshold && dBodyGetAngularDampingThreshold(b[i]) == (dReal)expected[i].ang_threshold);
            EXPECT(dBodyGetMaxAngularSpeed(b[i]) == (dReal)expected[i].max_angular_speed);
        }
    }
    for (i = 0; i < NB; i++) {
        dBodySetPosition(b[i], POS[i][0], POS[i][1], POS[i][2]);
        dBodySetLinearVel(b[i], LVEL[i][0], LVEL[i][1], LVEL[i][2]);
        dBodySetAngularVel(b[i], AVEL[i][0], AVEL[i][1], AVEL[i][2]);
    }
    dBodySetKinematic(b[NB - 1]);
    for (t = 0; t < TICKS; t++) {
        dContact c[NC];
        if (grow && t == GROW_AT)
            for (i = 0; i < NF; i++) {
                b[nb] = dBodyCreate(w);
                dBodySetPosition(b[nb], (dReal)(2 * i), 50, 20);
                dBodySetAngularVel(b[nb], 0, (dReal)(2 + i % 7), 0);
                nb++;
            }
        memset(c, 0, sizeof c);
        for (k = 0; k < NC; k++) {
            dJointID j;
            c[k].surface.mode = CON[k].bounce ? dContactBounce : 0;
            c[k].surface.mu = dInfinity; c[k].surface.bounce = (dReal)0.5; c[k].surface.bounce_vel = (dReal)0.1;
            for (i = 0; i < 3; i++) c[k].geom.pos[i] = POS[CON[k].body][i] + CON[k].off[i];
            c[k].geom.normal[1] = 1;
            c[k].geom.depth = CON[k].depth;
            j = dJointCreateContact(w, group, &c[k]);
            dJointAttach(j, b[CON[k].body], 0);
        }
        EXPECT((quick ? dWorldQuickStep(w, H) : dWorldStep(w, H)) == 1);
        dJointGroupEmpty(group);
        for (i = 0; i < nb; i++) {
            double s[13];
            const dReal *p, *q, *v, *a;
            if (i > NB && i != nb - 1) continue;
            p = dBodyGetPosition(b[i]); q = dBodyGetQuaternion(b[i]); v = dBodyGetLinearVel(b[i]); a = dBodyGetAngularVel(b[i]);
            for (k = 0; k < 3; k++) { s[k] = p[k]; s[7 + k] = v[k]; s[10 + k] = a[k]; }
            for (k = 0; k < 4; k++) s[3 + k] = q[k];
            print_state(s);
        }
    }
    dJointGroupDestroy(group);
    dWorldDestroy(w);
    dCloseODE();
    return failures ? 1 : 0;
}

static int run_batch(int quick, int plain)
{
    static dReal state[MAXCAP * 13], one[MAXCAP], three[MAXCAP * 3], zero[MAXCAP * 3];
    static uint8_t flags[MAXCAP];
    static dmxBodyDamping table[MAXCAP];
    const int cap = grow ? MAXCAP : CAPACITY;
    const dmxBodyDamping def = { 0.0, 0.0, 0.01, 0.01, (double)INFINITY };
    dmxBatchID b;
    int i, k, t, nb = NB;
    MUST(dmxBatchCreate(&b, cap, sizeof(dReal) == 4 ? DMX_F32 : DMX_F64, 0));
    for (i = 0; i < cap; i++) {
        for (k = 0; k < 13; k++) state[i * 13 + k] = (dReal)(k == 3);          /* an empty slot: unit quaternion, unit mass */
        one[i] = 1; three[3 * i] = three[3 * i + 1] = three[3 * i + 2] = 1;
        flags[i] = 0; table[i] = def;
    }
    for (i = 0; i < NB; i++) {
        for (k = 0; k < 3; k++) { state[i * 13 + k] = POS[i][k]; state[i * 13 + 7 + k] = LVEL[i][k]; state[i * 13 + 10 + k] = AVEL[i][k]; }
        flags[i] = DMX_BODY_ALIVE;
        table[i] = expected[i];
    }
    flags[NB - 1] |= DMX_BODY_KINEMATIC;
    MUST(dmxBatchUpload(b, DMX_STATE, state, 0, cap));
    MUST(dmxBatchUpload(b, DMX_MASS, one, 0, cap));
    MUST(dmxBatchUpload(b, DMX_INERTIA, three, 0, cap));
    MUST(dmxBatchUpload(b, DMX_FORCE, zero, 0, cap));
    MUST(dmxBatchUpload(b, DMX_TORQUE, zero, 0, cap));
    MUST(dmxBatchUploadBodyFlags(b, flags, 0, cap));
    MUST(dmxBatchSetGravity(b, 0, (dReal)-9.8, 0));
    MUST(dmxBatchSetERP(b, (dReal)0.2));
    MUST(dmxBatchSetCFM(b, (dReal)1e-5));
    MUST(dmxBatchSetQuickStep(b, 20, (dReal)1.3));
    MUST(dmxBatchSetStepper(b, quick ? DMX_STEPPER_QUICK : DMX_STEPPER_EXACT));
    if (!plain) {
        double layer = -1, vmax = -1;
        dmxBodyDamping back[NB];
        MUST(dmxBatchUploadBodyDamping(b, table, 0, cap));
        MUST(dmxBatchSetContactCorrection(b, LAYER, VMAX));
        MUST(dmxBatchGetContactCorrection(b, &layer, &vmax));
        EXPECT(layer == (double)LAYER && vmax == (double)VMAX);
        MUST(dmxBatchDownloadBodyDamping(b, back, 0, NB));
        EXPECT(memcmp(back, expected, sizeof back) == 0);
    }
    for (t = 0; t < TICKS; t++) {
        dmxContactJoint c[NC];
        if (grow && t == GROW_AT) {
            /* what the ODE world does when it outgrows its batch: every slot's state, flags and table entry again */
            MUST(dmxBatchDownload(b, DMX_STATE, state, 0, NB));
            for (i = 0; i < NF; i++, nb++) {
                state[nb * 13 + 0] = (dReal)(2 * i); state[nb * 13 + 1] = 50; state[nb * 13 + 2] = 20;
                state[nb * 13 + 11] = (dReal)(2 + i % 7);
                flags[nb] = DMX_BODY_ALIVE;
                if (!plain) {
                    table[nb].lin_scale = (dReal)0.0625; table[nb].ang_scale = (dReal)0.125;
                    table[nb].lin_threshold = (dReal)0.25; table[nb].ang_threshold = (dReal)0.375; table[nb].max_angular_speed = (dReal)1.5;
                }
            }
            MUST(dmxBatchUpload(b, DMX_STATE, state, 0, cap));
            MUST(dmxBatchUploadBodyFlags(b, flags, 0, cap));
            if (!plain) MUST(dmxBatchUploadBodyDamping(b, table, 0, cap));
        }
        memset(c, 0, sizeof c);
        for (k = 0; k < NC; k++) {
            for (i = 0; i < 3; i++) c[k].pos[i] = (dReal)(POS[CON[k].body][i] + CON[k].off[i]);
            c[k].normal[1] = 1;
            c[k].depth = CON[k].depth;
            c[k].body1 = CON[k].body; c[k].body2 = -1;
            c[k].mode = CON[k].bounce ? DMX_CONTACT_BOUNCE : 0;
            c[k].mu = (double)INFINITY; c[k].bounce = (dReal)0.5; c[k].bounce_vel = (dReal)0.1;
        }
        MUST(dmxBatchStepJoints(b, H, NC, c));
        MUST(dmxBatchDownload(b, DMX_STATE, state, 0, nb));
        for (i = 0; i < nb; i++) {
            double s[13];
            if (i > NB && i != nb - 1) continue;
            for (k = 0; k < 13; k++) s[k] = state[i * 13 + k];
            print_state(s);
        }
    }
    MUST(dmxBatchDestroy(b));
    return failures ? 1 : 0;
}

int main(int argc, char **argv)
{
    int i, quick, plain;
    if (argc < 3) { fprintf(stderr, "usage: stability_tick_harness ode|batch step|quick [plain|grow]\n"); return 2; }
    quick = strcmp(argv[2], "quick") == 0;
    plain = argc > 3 && strcmp(argv[3], "plain") == 0;
    grow = argc > 3 && strcmp(argv[3], "grow") == 0;
    /* what the ODE calls of run_ode come to: body 0 the world's values with its own angular scale, 1 and 2 and 4 overridden */
    for (i = 0; i < NB; i++) {
        expected[i].lin_scale = (dReal)0.0625; expected[i].ang_scale = (dReal)0.125;
        expected[i].lin_threshold = (dReal)0.25; expected[i].ang_threshold = (dReal)0.375; expected[i].max_angular_speed = (dReal)1.5;
    }
    expected[0].ang_scale = (dReal)0.25;
    expected[1].lin_scale = (dReal)0.5; expected[1].ang_scale = 0; expected[1].lin_threshold = (dReal)0.125;
    expected[2].ang_threshold = (dReal)0.0625; expected[2].max_angular_speed = (double)INFINITY;
    expected[4].max_angular_speed = (dReal)0.75;
    if (strcmp(argv[1], "ode") == 0) return run_ode(quick, plain);
    if (strcmp(argv[1], "batch") == 0) return run_batch(quick, plain);
    fprintf(stderr, "stability_tick_harness: unknown mode %s\n", argv[1]);
    return 2;
}
