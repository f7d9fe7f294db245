/*
 * surface_ode_harness.c -- dContactMu2 / FDir1 / Motion1 / 2 / N / Slip1 / 2 through include/ode/ode.h, and the same scene through
 * include/dmx_batch.h (dmxBatchStepJointsSurface): a plain C99 client of both headers, built once per width of dReal (-DdDOUBLE
 * against libode_mi355, -DdSINGLE against libode_mi355_single), for tests/test_gpu_surface_ode.py.
 *
 *   surface_ode_harness ode|batch step|quick belt|slip|mix|plain
 * One box of mass 1 on the ground, four explicit contact joints per tick under its lower corners (depth 0, normal +y), attached in
 * turn as (box, world) and as (world, box) with the normal reversed.
 * belt   dContactMotion1 | dContactFDir1, fdir1 = +x, motion1 = BELT, mu = inf
 * slip   dContactSlip1 | dContactFDir1, fdir1 = +x, slip1 = SLIP, mu = inf, and dBodyAddForce(PUSH, 0, 0) before every tick
 * mix    per contact one of: Mu2 | FDir1 (0.5 / 0.2), Motion1 | Motion2 | FDir1, MotionN, Slip1 | Slip2 with mu = inf; the box moves
 * plain  none of the seven bits: the ODE face must make the call it always made, and the twin calls dmxBatchStepJoints
 * ode: the ODE calls.  batch: the twin -- the same uploads dWorldStep makes and the same contacts through the batch interface.
 * Both print, per tick, 13 numbers (%.17g): pos3 quat4 lvel3 avel3.  The test compares the two outputs as text.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include "dmx_batch.h"
#include "ode/ode.h"

#define NC 4
#define TICKS 60
#define CAPACITY 512            /* dWorldCreate's first batch */
#define H ((dReal)(1.0 / 60.0))
#define BELT ((dReal)0.5)
#define SLIP ((dReal)0.05)
#define PUSH ((dReal)3)

enum { BELT_SCENE, SLIP_SCENE, MIX_SCENE, PLAIN_SCENE };
static int scene;
#define MUST(call) do { int rc_ = (call); if (rc_ != DMX_OK) { printf("FAIL %s -> %d\n", #call, rc_); return 1; } } while (0)

static const dReal OFF[NC][3] = { { -0.5f, -0.5f, -0.5f }, { 0.5f, -0.5f, -0.5f }, { 0.5f, -0.5f, 0.5f }, { -0.5f, -0.5f, 0.5f } };

/* contact k of the scene: the surface and fdir1 (the geometry is the caller's) */
static void surface_of(int k, dContact *c)
{
    memset(c, 0, sizeof *c);
    c->surface.mu = dInfinity;
    c->fdir1[0] = 1;
    /* fields no bit selects carry values that would show if they were read */
    c->surface.mu2 = 7; c->surface.motion1 = 5; c->surface.motion2 = -5; c->surface.motionN = 3; c->surface.slip1 = (dReal)0.9; c->surface.slip2 = (dReal)0.8;
    if (scene == BELT_SCENE) { c->surface.mode = dContactMotion1 | dContactFDir1; c->surface.motion1 = BELT; }
    else if (scene == SLIP_SCENE) { c->surface.mode = dContactSlip1 | dContactFDir1; c->surface.slip1 = SLIP; }
    else if (scene == MIX_SCENE) {
        if (k == 0) { c->surface.mode = dContactMu2 | dContactFDir1; c->surface.mu = (dReal)0.5; c->surface.mu2 = (dReal)0.2; }
        else if (k == 1) { c->surface.mode = dContactMotion1 | dContactMotion2 | dContactFDir1; c->surface.mu = (dReal)0.5; c->surface.motion1 = (dReal)0.3; c->surface.motion2 = (dReal)-0.2; }
        else if (k == 2) { c->surface.mode = dContactMotionN; c->surface.mu = (dReal)0.5; c->surface.motionN = (dReal)0.1; }
        else { c->surface.mode = dContactSlip1 | dContactSlip2; c->surface.slip1 = (dReal)0.02; c->surface.slip2 = (dReal)0.05; }
    }
}

static void print_state(const double s[13])
{
    int k;
    for (k = 0; k < 13; k++) printf("%.17g%c", s[k], k == 12 ? '\n' : ' ');
}

static int run_ode(int quick)
{
    dWorldID w;
    dJointGroupID group;
    dBodyID b;
    int i, k, t;
    dInitODE();
    w = dWorldCreate();
    group = dJointGroupCreate(0);
    dWorldSetGravity(w, 0, (dReal)-9.8, 0);
    dWorldSetCFM(w, (dReal)1e-5);
    b = dBodyCreate(w);
    dBodySetPosition(b, 0, (dReal)0.5, 0);
    if (scene == MIX_SCENE) { dBodySetLinearVel(b, (dReal)0.4, (dReal)-0.5, (dReal)0.3); dBodySetAngularVel(b, 0, (dReal)0.25, 0); }
    for (t = 0; t < TICKS; t++) {
        dContact c[NC];
        const dReal *x = dBodyGetPosition(b);
        for (k = 0; k < NC; k++) {
            dJointID j;
            const int world_first = k & 1;
            surface_of(k, &c[k]);
            for (i = 0; i < 3; i++) c[k].geom.pos[i] = x[i] + OFF[k][i];
            c[k].geom.normal[1] = (dReal)(world_first ? -1 : 1);
            j = dJointCreateContact(w, group, &c[k]);
            if (world_first) dJointAttach(j, 0, b); else dJointAttach(j, b, 0);
        }
        if (scene == SLIP_SCENE) dBodyAddForce(b, PUSH, 0, 0);
        if ((quick ? dWorldQuickStep(w, H) : dWorldStep(w, H)) != 1) { printf("FAIL step\n"); return 1; }
        dJointGroupEmpty(group);
        {
            double s[13];
            const dReal *p = dBodyGetPosition(b), *q = dBodyGetQuaternion(b), *v = dBodyGetLinearVel(b), *a = dBodyGetAngularVel(b);
            for (k = 0; k < 3; k++) { s[k] = p[k]; s[7 + k] = v[k]; s[10 + k] = a[k]; }
            for (k = 0; k < 4; k++) s[3 + k] = q[k];
            print_state(s);
        }
    }
    dJointGroupDestroy(group);
    dWorldDestroy(w);
    dCloseODE();
    return 0;
}

static int run_batch(int quick)
{
    static dReal state[CAPACITY * 13], one[CAPACITY], three[CAPACITY * 3], zero[CAPACITY * 3];
    static uint8_t flags[CAPACITY];
    dmxBatchID b;
    int i, k, t;
    MUST(dmxBatchCreate(&b, CAPACITY, sizeof(dReal) == 4 ? DMX_F32 : DMX_F64, 0));
    for (i = 0; i < CAPACITY; i++) {
        for (k = 0; k < 13; k++) state[i * 13 + k] = (dReal)(k == 3);          /* an empty slot: unit quaternion, unit mass */
        one[i] = 1; three[3 * i] = three[3 * i + 1] = three[3 * i + 2] = 1;
        flags[i] = 0;
    }
    state[1] = (dReal)0.5;
    if (scene == MIX_SCENE) { state[7] = (dReal)0.4; state[8] = (dReal)-0.5; state[9] = (dReal)0.3; state[11] = (dReal)0.25; }
    flags[0] = DMX_BODY_ALIVE;
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
    for (t = 0; t < TICKS; t++) {
        dmxContactJoint c[NC];
        dmxContactSurface s[NC];
        memset(c, 0, sizeof c);
        memset(s, 0, sizeof s);
        MUST(dmxBatchDownload(b, DMX_STATE, state, 0, 1));
        for (k = 0; k < NC; k++) {
            dContact ct;
            const int world_first = k & 1;
            surface_of(k, &ct);
            for (i = 0; i < 3; i++) { c[k].pos[i] = (dReal)(state[i] + OFF[k][i]); s[k].fdir1[i] = ct.fdir1[i]; }
            c[k].normal[1] = world_first ? -1 : 1;
            c[k].body1 = world_first ? -1 : 0; c[k].body2 = world_first ? 0 : -1;
            c[k].mode = ct.surface.mode; c[k].mu = ct.surface.mu;
            s[k].mu2 = ct.surface.mu2; s[k].motion1 = ct.surface.motion1; s[k].motion2 = ct.surface.motion2; s[k].motionN = ct.surface.motionN;
            s[k].slip1 = ct.surface.slip1; s[k].slip2 = ct.surface.slip2;
        }
        if (scene == SLIP_SCENE) { dReal f[3] = { PUSH, 0, 0 }; MUST(dmxBatchUpload(b, DMX_FORCE, f, 0, 1)); }
        if (scene == PLAIN_SCENE) MUST(dmxBatchStepJoints(b, H, NC, c));
        else MUST(dmxBatchStepJointsSurface(b, H, NC, c, s));
        MUST(dmxBatchDownload(b, DMX_STATE, state, 0, 1));
        {
            double out[13];
            for (k = 0; k < 13; k++) out[k] = state[k];
            print_state(out);
        }
    }
    MUST(dmxBatchDestroy(b));
    return 0;
}

int main(int argc, char **argv)
{
    int quick;
    if (argc != 4) { fprintf(stderr, "usage: surface_ode_harness ode|batch step|quick belt|slip|mix|plain\n"); return 2; }
    quick = strcmp(argv[2], "quick") == 0;
    scene = strcmp(argv[3], "belt") == 0 ? BELT_SCENE : strcmp(argv[3], "slip") == 0 ? SLIP_SCENE : strcmp(argv[3], "mix") == 0 ? MIX_SCENE : PLAIN_SCENE;
    return strcmp(argv[1], "ode") == 0 ? run_ode(quick) : run_batch(quick);
}
