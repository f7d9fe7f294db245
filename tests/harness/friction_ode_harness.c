/* friction_ode_harness.c -- a box dropped flat on the ground plane, friction bounded by the normal force (dContactApprox1), through
 * the ODE calls of include/ode/ode.h alone; links against either shipped library (-DdSINGLE: libode_mi355_single).
 *
 *   friction_ode_harness <tan_theta> <quick: 0 | 1> <ticks>
 * Gravity is 9.8 tilted by theta towards +x.  Per tick it prints one line
 *   T pos3 quat4 lvel3 avel3 | n | n x (pos3 normal3 depth side) | lvel3 avel3
 * : the box before the tick, the contacts the near callback saw (side 1: the box is the contact's first body, 2: its second), and the
 * box's velocities after the tick, at 17 significant digits. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <ode/ode.h>

#define MAXC 8
static dWorldID world;
static dJointGroupID group;
static dBodyID box;
static int n_seen;
static double seen[MAXC * 2][8];

static void near_cb(void *data, dGeomID o1, dGeomID o2)
{
    dContact c[MAXC];
    int k, d, n = dCollide(o1, o2, MAXC, &c[0].geom, sizeof(dContact));
    (void)data;
    for (k = 0; k < n; k++) {
        dBodyID b1 = dGeomGetBody(o1), b2 = dGeomGetBody(o2);
        c[k].surface.mode = dContactApprox1;
        c[k].surface.mu = (dReal)0.5;
        dJointAttach(dJointCreateContact(world, group, &c[k]), b1, b2);
        if (n_seen < MAXC * 2) {
            for (d = 0; d < 3; d++) { seen[n_seen][d] = c[k].geom.pos[d]; seen[n_seen][3 + d] = c[k].geom.normal[d]; }
            seen[n_seen][6] = c[k].geom.depth;
            seen[n_seen][7] = b1 == box ? 1 : 2;
            n_seen++;
        }
    }
}

static void print_n(const dReal *v, int n) { int k; for (k = 0; k < n; k++) printf(" %.17g", (double)v[k]); }

int main(int argc, char **argv)
{
    double tan_theta, theta;
    int quick, ticks, t, k, d;
    dSpaceID space;
    dGeomID g;
    dMass m;
    if (argc != 4) { fprintf(stderr, "usage: friction_ode_harness <tan_theta> <quick> <ticks>\n"); return 2; }
    tan_theta = atof(argv[1]); quick = atoi(argv[2]); ticks = atoi(argv[3]);
    theta = atan(tan_theta);
    dInitODE();
    world = dWorldCreate();
    dWorldSetGravity(world, (dReal)(9.8 * sin(theta)), (dReal)(-9.8 * cos(theta)), 0);
    dWorldSetCFM(world, (dReal)1e-5);
    dWorldSetERP(world, (dReal)0.2);
    space = dSimpleSpaceCreate(0);
    group = dJointGroupCreate(0);
    dCreatePlane(space, 0, 1, 0, 0);
    box = dBodyCreate(world);
    dMassSetBoxTotal(&m, 2, 1, 1, 1);
    dBodySetMass(box, &m);
    dBodySetPosition(box, 0, (dReal)0.55, 0);
    g = dCreateBox(space, 1, 1, 1);
    dGeomSetBody(g, box);
    for (t = 0; t < ticks; t++) {
        printf("T");
        print_n(dBodyGetPosition(box), 3); print_n(dBodyGetQuaternion(box), 4);
        print_n(dBodyGetLinearVel(box), 3); print_n(dBodyGetAngularVel(box), 3);
        n_seen = 0;
        dSpaceCollide(space, 0, near_cb);
        printf(" | %d |", n_seen);
        for (k = 0; k < n_seen; k++) for (d = 0; d < 8; d++) printf(" %.17g", seen[k][d]);
        if ((quick ? dWorldQuickStep(world, (dReal)(1.0 / 60.0)) : dWorldStep(world, (dReal)(1.0 / 60.0))) != 1) { fprintf(stderr, "step failed\n"); return 1; }
        dJointGroupEmpty(group);
        printf(" |");
        print_n(dBodyGetLinearVel(box), 3); print_n(dBodyGetAngularVel(box), 3);
        printf("\n");
    }
    dWorldDestroy(world);
    dCloseODE();
    return 0;
}
