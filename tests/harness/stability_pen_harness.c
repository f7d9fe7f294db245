/*
 * stability_pen_harness.c -- tests/harness/autodisable_tick_harness.c (the reference's tick loop through include/ode/ode.h with
 * auto-disable: same scene on stdin, same HARNESS_* switches, same report) with the world's damping and contact correction set
 * right after dWorldCreate, as an ODE program sets them, for scripts/time_stability.py:
 *
 *   HARNESS_DAMPING="lin ang"         dWorldSetDamping(world, lin, ang) before any body is made (the bodies inherit it)
 *   HARNESS_SURFACE_LAYER=depth       dWorldSetContactSurfaceLayer(world, depth)
 *   HARNESS_MAX_CORRECTING_VEL=vel    dWorldSetContactMaxCorrectingVel(world, vel)
 *   HARNESS_MAX_ANGULAR_SPEED=speed   dWorldSetMaxAngularSpeed(world, speed)
 *
 * The tick loop is that file's own, included below with its dWorldCreate sent through the function that makes these calls.
 */
#define _POSIX_C_SOURCE 199309L     /* (that file's own first line: clock_gettime) */
#include <stdio.h>
#include <stdlib.h>
#include <ode/ode.h>

static dWorldID stability_world_create(void)
{
    dWorldID w = dWorldCreate();
    double a, b;
    if (getenv("HARNESS_DAMPING")) {
        if (sscanf(getenv("HARNESS_DAMPING"), "%lf %lf", &a, &b) != 2) { fprintf(stderr, "harness: bad HARNESS_DAMPING\n"); exit(2); }
        dWorldSetDamping(w, (dReal)a, (dReal)b);
    }
    if (getenv("HARNESS_SURFACE_LAYER")) dWorldSetContactSurfaceLayer(w, (dReal)atof(getenv("HARNESS_SURFACE_LAYER")));
    if (getenv("HARNESS_MAX_CORRECTING_VEL")) dWorldSetContactMaxCorrectingVel(w, (dReal)atof(getenv("HARNESS_MAX_CORRECTING_VEL")));
    if (getenv("HARNESS_MAX_ANGULAR_SPEED")) dWorldSetMaxAngularSpeed(w, (dReal)atof(getenv("HARNESS_MAX_ANGULAR_SPEED")));
    return w;
}

#define dWorldCreate stability_world_create
#include "autodisable_tick_harness.c"
