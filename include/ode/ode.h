/*
 * include/ode/ode.h -- the ODE C API subset that /root/reference/src/main.c
 * links against (33 symbols), plus the few neighbours the
 * BASELINE.json scenes need (dWorldQuickStep, dCreatePlane, dBodySetMass,
 * dMassSetBox ...).  Served by libode_mi355.so: object bookkeeping, the
 * broadphase callback loop and dCollide run on the host (the API is a
 * synchronous per-pair host callback, main.c:212, 674-693); the step itself --
 * contact rows, SOR, integration -- runs on the MI355X.  Each declaration
 * cites the reference call site it serves.
 *
 * dWorldStep (main.c:213) solves every island's boxed LCP to the end -- the
 * solution ODE's Dantzig solver reaches, by block principal pivoting on the
 * device -- and dWorldQuickStep runs QuickStep's 20 SOR sweeps: the two names
 * behave as ODE's two steppers do.
 * Errors: no call site checks a return value (main.c:94-98, 212-214); failures
 * print to stderr and return 0 / NULL, HIP failures abort like ODE's dError.
 */
#ifndef DMX_ODE_H
#define DMX_ODE_H

#include <stddef.h>
#include "common.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- contact structures (main.c:676-687) ---------------------------------
 * Layout and flag values are those of the ODE 0.13 - 0.16 line's ode/contact.h [ODE-recall; SURVEY.md cites 0.16.x]: rolling
 * friction (rho, rho2, rhoN; dContactRolling, dContactApprox1_N) sits between mu2 and bounce, so an object compiled against
 * stock 0.16 headers writes `bounce` where this library reads it (tests/test_ode_compat.py checks every offset).  ODE <= 0.12
 * had no rho fields: objects built against those headers must be recompiled against these.  The rolling-friction fields are
 * accepted and ignored (the reference never sets them, main.c:684-687).  dContactMu2, dContactFDir1, dContactMotion1 / 2 / N and
 * dContactSlip1 / 2 are honoured, by the definition of include/dmx_batch.h at DMX_CONTACT_MU2. */
enum {
    dContactMu2      = 0x001,
    dContactAxisDep  = 0x001,
    dContactFDir1    = 0x002,
    dContactBounce   = 0x004,   /* main.c:684 */
    dContactSoftERP  = 0x008,
    dContactSoftCFM  = 0x010,
    dContactMotion1  = 0x020,
    dContactMotion2  = 0x040,
    dContactMotionN  = 0x080,
    dContactSlip1    = 0x100,
    dContactSlip2    = 0x200,
    dContactRolling  = 0x400,
    dContactApprox0  = 0x0000,
    dContactApprox1_1 = 0x1000,
    dContactApprox1_2 = 0x2000,
    dContactApprox1_N = 0x4000,
    dContactApprox1  = 0x7000
};

typedef struct dSurfaceParameters {
    int mode;                 /* main.c:684 */
    dReal mu;                 /* main.c:687 */
    dReal mu2;
    dReal rho, rho2, rhoN;    /* rolling / spinning friction (0.13+): not used by the reference, ignored here */
    dReal bounce;             /* main.c:685 */
    dReal bounce_vel;         /* main.c:686 */
    dReal soft_erp;
    dReal soft_cfm;
    dReal motion1, motion2, motionN;
    dReal slip1, slip2;
} dSurfaceParameters;

typedef struct dContactGeom {
    dVector3 pos;
    dVector3 normal;          /* points into body 1 */
    dReal depth;
    dGeomID g1, g2;
    int side1, side2;
} dContactGeom;

typedef struct dContact {
    dSurfaceParameters surface;
    dContactGeom geom;        /* &contacts[0].geom with stride sizeof(dContact): main.c:678 */
    dVector3 fdir1;
} dContact;

typedef void dNearCallback(void *data, dGeomID o1, dGeomID o2);   /* main.c:48, 674 */

typedef struct dMass {
    dReal mass;
    dVector3 c;
    dMatrix3 I;
} dMass;

enum { dSphereClass = 0, dBoxClass = 1, dPlaneClass = 4, dRayClass = 5 };

/* ---- library lifecycle ---------------------------------------------------- */
void dInitODE(void);                                             /* main.c:94  */
int  dInitODE2(unsigned int flags);
void dCloseODE(void);                                            /* main.c:267 */

/* ---- world ---------------------------------------------------------------- */
dWorldID dWorldCreate(void);                                     /* main.c:95  */
void dWorldDestroy(dWorldID);                                    /* main.c:266 */
void dWorldSetGravity(dWorldID, dReal x, dReal y, dReal z);      /* main.c:96  */
void dWorldGetGravity(dWorldID, dVector3 gravity);
void dWorldSetERP(dWorldID, dReal erp);
dReal dWorldGetERP(dWorldID);
void dWorldSetCFM(dWorldID, dReal cfm);
dReal dWorldGetCFM(dWorldID);
void dWorldSetQuickStepNumIterations(dWorldID, int num);
int  dWorldGetQuickStepNumIterations(dWorldID);
void dWorldSetQuickStepW(dWorldID, dReal over_relaxation);
dReal dWorldGetQuickStepW(dWorldID);
/* Auto-disable: a body whose speeds have stayed under the thresholds for the idle steps and the idle time is put to sleep; an
 * island without an awake body is not stepped; a sleeping body wakes when something awake becomes connected to it (the rule is
 * in include/dmx_batch.h, "auto-disable").  Off by default, as in ODE; defaults 0.01, 0.01, 10 steps, 0 s [ODE-recall].
 * Departures from ODE: the four values are the world's and hold for ALL its bodies from the next step on (ODE copies them into a
 * body at creation), and setting one resets every body's idle counters; there are no per-body thresholds; the idle test looks at
 * the step's own velocities (an average samples count other than 1 is refused with one line on stderr); the test runs at the end
 * of the step, not at the start of the next.  dBodySetPosition, dBodyAddForce and the like do not wake a body [ODE-recall];
 * dBodyEnable does.  dSpaceCollide hands pairs of disabled bodies to the callback like any other [ODE-recall]. */
void dWorldSetAutoDisableFlag(dWorldID, int do_auto_disable);     /* what dBodyCreate copies into a new body */
int  dWorldGetAutoDisableFlag(dWorldID);
void dWorldSetAutoDisableLinearThreshold(dWorldID, dReal linear_threshold);
dReal dWorldGetAutoDisableLinearThreshold(dWorldID);
void dWorldSetAutoDisableAngularThreshold(dWorldID, dReal angular_threshold);
dReal dWorldGetAutoDisableAngularThreshold(dWorldID);
void dWorldSetAutoDisableSteps(dWorldID, int steps);
int  dWorldGetAutoDisableSteps(dWorldID);
void dWorldSetAutoDisableTime(dWorldID, dReal time);
dReal dWorldGetAutoDisableTime(dWorldID);
void dWorldSetAutoDisableAverageSamplesCount(dWorldID, unsigned int average_samples_count);   /* 1 only */
int  dWorldGetAutoDisableAverageSamplesCount(dWorldID);
/* damping, maximum angular speed and the contact correction scalars (include/dmx_batch.h, "damping"): all no-ops at their defaults,
 * scale 0, thresholds 0.01, maximum speed dInfinity, layer 0, maximum correcting velocity dInfinity.  The world's damping values
 * and maximum angular speed are what dBodyCreate copies into a new body; bodies that exist keep theirs.  A value out of range
 * (a scale outside [0, 1], a negative threshold or layer, a maximum that is not positive) is ignored with one line on stderr.
 * Unlike stock ODE, kinematic bodies are not damped. */
void dWorldSetLinearDamping(dWorldID, dReal scale);
dReal dWorldGetLinearDamping(dWorldID);
void dWorldSetAngularDamping(dWorldID, dReal scale);
dReal dWorldGetAngularDamping(dWorldID);
void dWorldSetDamping(dWorldID, dReal linear_scale, dReal angular_scale);
void dWorldSetLinearDampingThreshold(dWorldID, dReal threshold);
dReal dWorldGetLinearDampingThreshold(dWorldID);
void dWorldSetAngularDampingThreshold(dWorldID, dReal threshold);
dReal dWorldGetAngularDampingThreshold(dWorldID);
void dWorldSetMaxAngularSpeed(dWorldID, dReal max_speed);
dReal dWorldGetMaxAngularSpeed(dWorldID);
void dWorldSetContactSurfaceLayer(dWorldID, dReal depth);
dReal dWorldGetContactSurfaceLayer(dWorldID);
void dWorldSetContactMaxCorrectingVel(dWorldID, dReal vel);
dReal dWorldGetContactMaxCorrectingVel(dWorldID);
int  dWorldStep(dWorldID, dReal stepsize);                       /* main.c:213 */
int  dWorldQuickStep(dWorldID, dReal stepsize);

/* ---- bodies --------------------------------------------------------------- */
dBodyID dBodyCreate(dWorldID);                                   /* main.c:703 */
void dBodyDestroy(dBodyID);                                      /* main.c:261 */
void dBodySetPosition(dBodyID, dReal x, dReal y, dReal z);       /* main.c:708 */
void dBodySetRotation(dBodyID, const dMatrix3 R);                /* main.c:709 */
void dBodySetQuaternion(dBodyID, const dQuaternion q);
void dBodySetLinearVel(dBodyID, dReal x, dReal y, dReal z);
void dBodySetAngularVel(dBodyID, dReal x, dReal y, dReal z);
const dReal *dBodyGetPosition(dBodyID);                          /* main.c:229 */
const dReal *dBodyGetRotation(dBodyID);                          /* main.c:230 */
const dReal *dBodyGetQuaternion(dBodyID);
const dReal *dBodyGetLinearVel(dBodyID);
const dReal *dBodyGetAngularVel(dBodyID);
void dBodySetKinematic(dBodyID);                                 /* main.c:712 */
void dBodySetDynamic(dBodyID);
int  dBodyIsKinematic(dBodyID);
void dBodySetAutoDisableFlag(dBodyID, int do_auto_disable);      /* 0 also enables the body [ODE-recall] */
int  dBodyGetAutoDisableFlag(dBodyID);
void dBodySetAutoDisableDefaults(dBodyID);                       /* the world's flag */
void dBodyEnable(dBodyID);                                       /* wakes the body and resets its idle counters */
void dBodyDisable(dBodyID);                                      /* asleep from the next step on, velocities as they are */
int  dBodyIsEnabled(dBodyID);
void dBodySetLinearDamping(dBodyID, dReal scale);
dReal dBodyGetLinearDamping(dBodyID);
void dBodySetAngularDamping(dBodyID, dReal scale);
dReal dBodyGetAngularDamping(dBodyID);
void dBodySetDamping(dBodyID, dReal linear_scale, dReal angular_scale);
void dBodySetLinearDampingThreshold(dBodyID, dReal threshold);
dReal dBodyGetLinearDampingThreshold(dBodyID);
void dBodySetAngularDampingThreshold(dBodyID, dReal threshold);
dReal dBodyGetAngularDampingThreshold(dBodyID);
void dBodySetMaxAngularSpeed(dBodyID, dReal max_speed);
dReal dBodyGetMaxAngularSpeed(dBodyID);
void dBodySetDampingDefaults(dBodyID);                           /* the world's five values */
void dBodyAddForce(dBodyID, dReal fx, dReal fy, dReal fz);       /* main.c:532 (commented out there) */
void dBodyAddTorque(dBodyID, dReal fx, dReal fy, dReal fz);
void dBodySetMass(dBodyID, const dMass *mass);
void dBodyGetMass(dBodyID, dMass *mass);
void dBodySetGyroscopicMode(dBodyID, int enabled);
int  dBodyGetGyroscopicMode(dBodyID);
dWorldID dBodyGetWorld(dBodyID);

void dMassSetZero(dMass *);
void dMassSetParameters(dMass *, dReal themass, dReal cgx, dReal cgy, dReal cgz,
                        dReal I11, dReal I22, dReal I33, dReal I12, dReal I13, dReal I23);
void dMassSetBox(dMass *, dReal density, dReal lx, dReal ly, dReal lz);
void dMassSetBoxTotal(dMass *, dReal total_mass, dReal lx, dReal ly, dReal lz);
void dMassSetSphere(dMass *, dReal density, dReal radius);
void dMassSetSphereTotal(dMass *, dReal total_mass, dReal radius);

/* ---- spaces and geoms ----------------------------------------------------- */
dSpaceID dHashSpaceCreate(dSpaceID space);                       /* main.c:97  */
dSpaceID dSimpleSpaceCreate(dSpaceID space);
void dSpaceDestroy(dSpaceID);
void dSpaceCollide(dSpaceID space, void *data, dNearCallback *callback);   /* main.c:212 */
int  dSpaceGetNumGeoms(dSpaceID);

dGeomID dCreateBox(dSpaceID space, dReal lx, dReal ly, dReal lz);          /* main.c:720, 743 */
dGeomID dCreateSphere(dSpaceID space, dReal radius);                       /* main.c:717 */
dGeomID dCreatePlane(dSpaceID space, dReal a, dReal b, dReal c, dReal d);
void dGeomDestroy(dGeomID);                                      /* main.c:263 */
void dGeomSetBody(dGeomID, dBodyID);                             /* main.c:726 */
dBodyID dGeomGetBody(dGeomID);                                   /* main.c:691 */
void dGeomSetPosition(dGeomID, dReal x, dReal y, dReal z);       /* main.c:748 */
void dGeomSetRotation(dGeomID, const dMatrix3 R);                /* main.c:749 */
const dReal *dGeomGetPosition(dGeomID);                          /* main.c:232 */
const dReal *dGeomGetRotation(dGeomID);                          /* main.c:233 */
void dGeomSetCategoryBits(dGeomID, unsigned long bits);          /* main.c:724, 751, 752 */
void dGeomSetCollideBits(dGeomID, unsigned long bits);           /* main.c:725 */
unsigned long dGeomGetCategoryBits(dGeomID);
unsigned long dGeomGetCollideBits(dGeomID);
int  dGeomGetClass(dGeomID);
void dGeomBoxGetLengths(dGeomID box, dVector3 result);
dReal dGeomSphereGetRadius(dGeomID sphere);
void dGeomPlaneGetParams(dGeomID plane, dVector4 result);

/* flags: low 16 bits = max contacts; skip = byte stride between dContactGeoms (main.c:678) */
int dCollide(dGeomID o1, dGeomID o2, int flags, dContactGeom *contact, int skip);

/* Rays: a bounded slice of ODE's ray geom.  dCreateRay supports space == 0 only -- a ray here does not take part in
 * dSpaceCollide (no near callback is ever called with one), so putting it into a space would promise what is not there: a
 * non-null space prints to stderr and returns 0.  The ray starts at its position and runs along the normalised direction for
 * `length`; dCollide(ray, g) and dCollide(g, ray) against a box, a sphere or a plane return at most one contact, g1 = the ray,
 * whichever order the geoms were given in: pos = the first crossing of g's surface, depth = its distance from the start, normal
 * = the surface's outward unit normal there, negated when the start lies inside g (what ODE's ray colliders return).  Runs
 * on the host, through the same primitives as dmxBatchRayCast (include/dmx_batch.h), the batch form of the query. */
dGeomID dCreateRay(dSpaceID space, dReal length);
void dGeomRaySet(dGeomID ray, dReal px, dReal py, dReal pz, dReal dx, dReal dy, dReal dz);
void dGeomRayGet(dGeomID ray, dVector3 start, dVector3 dir);
void dGeomRaySetLength(dGeomID ray, dReal length);
dReal dGeomRayGetLength(dGeomID ray);

/* ---- contact joints ------------------------------------------------------- */
dJointGroupID dJointGroupCreate(int max_size);                   /* main.c:98  */
void dJointGroupEmpty(dJointGroupID);                            /* main.c:214 */
void dJointGroupDestroy(dJointGroupID);                          /* main.c:265 */
dJointID dJointCreateContact(dWorldID, dJointGroupID, const dContact *);   /* main.c:690 */
void dJointAttach(dJointID, dBodyID body1, dBodyID body2);       /* main.c:691 */

/* ---- articulation joints: ball-and-socket, hinge, slider and fixed [ODE-recall objects.h].  Anchors and axes are given in world
 * coordinates after dJointAttach and kept in the bodies' frames at their poses of that moment; a body of 0 is the world.
 * dJointAttach(j, 0, body) exchanges the two, as ODE does: dJointGetBody(j, 0) is the body.  dWorldDestroy destroys the joints that
 * are in no group.  dBodyDestroy detaches the body's joints (both sides: the joint does nothing until it is attached again).
 * dWorldStep / dWorldQuickStep honour them (include/dmx_batch.h, dmxBatchSetJoints).
 * Hinges have limits, a motor, an angle and a rate (include/dmx_batch.h, dmxBatchSetHingeLimots): dJointSetHingeParam honours
 * dParamLoStop, dParamHiStop, dParamVel and dParamFMax -- fudge factor 1, no bounce, the world's ERP / CFM at the stops; the other
 * parameters print one line to stderr and are ignored on set, and read as 0.  dJointSetHingeAnchor / dJointSetHingeAxis take the
 * bodies' current relative pose as angle zero, as ODE does.  Angle, rate, stops, motor and dJointAddHingeTorque are those of the
 * sides as attached: body 1 relative to body 2 about the axis, also after dJointAttach(j, 0, body).  Balls have none of these. */
enum { dJointTypeNone = 0, dJointTypeBall = 1, dJointTypeHinge = 2, dJointTypeSlider = 3, dJointTypeContact = 4, dJointTypeFixed = 7,
       dJointTypeAMotor = 9 };
dJointID dJointCreateBall(dWorldID, dJointGroupID);
dJointID dJointCreateHinge(dWorldID, dJointGroupID);
dJointID dJointCreateSlider(dWorldID, dJointGroupID);
dJointID dJointCreateFixed(dWorldID, dJointGroupID);
void dJointDestroy(dJointID);
int dJointGetType(dJointID);
dBodyID dJointGetBody(dJointID, int index);
void dJointSetBallAnchor(dJointID, dReal x, dReal y, dReal z);
void dJointGetBallAnchor(dJointID, dVector3 result);
void dJointGetBallAnchor2(dJointID, dVector3 result);
void dJointSetHingeAnchor(dJointID, dReal x, dReal y, dReal z);
void dJointSetHingeAxis(dJointID, dReal x, dReal y, dReal z);
void dJointGetHingeAnchor(dJointID, dVector3 result);
void dJointGetHingeAnchor2(dJointID, dVector3 result);
void dJointGetHingeAxis(dJointID, dVector3 result);
/* [ODE-recall common.h D_ALL_PARAM_NAMES, 0.13 - 0.16] */
enum { dParamLoStop = 0, dParamHiStop, dParamVel, dParamLoVel, dParamHiVel, dParamFMax, dParamFudgeFactor, dParamBounce, dParamCFM,
       dParamStopERP, dParamStopCFM, dParamSuspensionERP, dParamSuspensionCFM, dParamERP };
/* the second and third axis of a joint with several (an angular motor): dParamXxx2 = dParamGroup + dParamXxx, dParamXxx3 = 2 dParamGroup + dParamXxx */
enum { dParamGroup = 0x100 };
enum { dParamLoStop1 = 0x000, dParamHiStop1, dParamVel1, dParamLoVel1, dParamHiVel1, dParamFMax1, dParamFudgeFactor1, dParamBounce1, dParamCFM1,
       dParamStopERP1, dParamStopCFM1, dParamSuspensionERP1, dParamSuspensionCFM1, dParamERP1 };
enum { dParamLoStop2 = 0x100, dParamHiStop2, dParamVel2, dParamLoVel2, dParamHiVel2, dParamFMax2, dParamFudgeFactor2, dParamBounce2, dParamCFM2,
       dParamStopERP2, dParamStopCFM2, dParamSuspensionERP2, dParamSuspensionCFM2, dParamERP2 };
enum { dParamLoStop3 = 0x200, dParamHiStop3, dParamVel3, dParamLoVel3, dParamHiVel3, dParamFMax3, dParamFudgeFactor3, dParamBounce3, dParamCFM3,
       dParamStopERP3, dParamStopCFM3, dParamSuspensionERP3, dParamSuspensionCFM3, dParamERP3 };
void dJointSetHingeParam(dJointID, int parameter, dReal value);
dReal dJointGetHingeParam(dJointID, int parameter);
dReal dJointGetHingeAngle(dJointID);
dReal dJointGetHingeAngleRate(dJointID);
void dJointAddHingeTorque(dJointID, dReal torque);
/* Sliders and fixed joints (include/dmx_batch.h, DMX_JOINT_SLIDER / DMX_JOINT_FIXED).  dJointSetSliderAxis takes the axis in world
 * coordinates, puts the anchor at body 1's centre (body 2's when body 1 is the world) and takes the current pose as the zero pose and
 * as position zero.  Position, rate, stops (metres), motor (m/s, N) and dJointAddSliderForce are those of the sides as attached:
 * the position grows when body 1 moves along the axis relative to body 2.  dJointSetSliderParam honours the four parameters
 * dJointSetHingeParam honours; the others print the same line and are ignored.  dJointAddSliderForce applies +f u to body 1 and -f u
 * to body 2, both at body 2's anchor point: the pair's momentum and angular momentum do not change.  dJointSetFixed welds the two
 * bodies at their current relative pose, the anchor at body 2's centre. */
void dJointSetSliderAxis(dJointID, dReal x, dReal y, dReal z);
void dJointGetSliderAxis(dJointID, dVector3 result);
dReal dJointGetSliderPosition(dJointID);
dReal dJointGetSliderPositionRate(dJointID);
void dJointSetSliderParam(dJointID, int parameter, dReal value);
dReal dJointGetSliderParam(dJointID, int parameter);
void dJointAddSliderForce(dJointID, dReal force);
void dJointSetFixed(dJointID);
/* Angular motors (include/dmx_batch.h, DMX_JOINT_AMOTOR), usually beside a ball joint on the same two bodies.  dAMotorUser: one to three
 * axes, each given in world coordinates and kept in the frame `rel` names (0: the world, 1: the first body, 2: the second), with the
 * angle the caller supplies (dJointSetAMotorAngle).  dAMotorEuler: three axes; axis 0 goes with the first body and axis 2 with the
 * second (they must be perpendicular when they are set), axis 1 and the three Euler angles are computed; the pose at which axis 0 or 2
 * is set, with both known, is angles zero.  Every axis has a stop and a motor: dJointSetAMotorParam honours dParamLoStop, dParamHiStop,
 * dParamVel and dParamFMax and their ...2 / ...3 groups; the other parameters print one line to stderr and are ignored on set, and read
 * as 0 (dParamFudgeFactor, dParamBounce, dParamCFM, dParamStopERP, dParamStopCFM: fudge 1, no bounce, the world's ERP / CFM, as for the
 * hinge).  dJointGetAMotorAngleRate is a_i . (omega_1 - omega_2), the velocity the axis's row acts on: the angle's own rate for the
 * middle Euler axis, for axes 0 and 2 only near a middle angle of 0.  Axes, angles, rates, stops, motors and dJointAddAMotorTorques
 * (+sum t_i a_i on the first body, the opposite on the second) are those of the sides as attached, also after dJointAttach(j, 0, body).
 * dJointSetFeedback reports torques only: the forces are zero.  Not provided: dJointCreateLMotor; an Euler-mode angle with the world
 * on both ends. */
enum { dAMotorUser = 0, dAMotorEuler = 1 };
dJointID dJointCreateAMotor(dWorldID, dJointGroupID);
void dJointSetAMotorMode(dJointID, int mode);
int dJointGetAMotorMode(dJointID);
void dJointSetAMotorNumAxes(dJointID, int num);
int dJointGetAMotorNumAxes(dJointID);
void dJointSetAMotorAxis(dJointID, int anum, int rel, dReal x, dReal y, dReal z);
void dJointGetAMotorAxis(dJointID, int anum, dVector3 result);
int dJointGetAMotorAxisRel(dJointID, int anum);
void dJointSetAMotorAngle(dJointID, int anum, dReal angle);
dReal dJointGetAMotorAngle(dJointID, int anum);
dReal dJointGetAMotorAngleRate(dJointID, int anum);
void dJointSetAMotorParam(dJointID, int parameter, dReal value);
dReal dJointGetAMotorParam(dJointID, int parameter);
void dJointAddAMotorTorques(dJointID, dReal torque1, dReal torque2, dReal torque3);
/* The force and torque a joint applied to its two bodies during the last dWorldStep / dWorldQuickStep, about each body's centre,
 * in world coordinates (ODE's layout and meaning; include/dmx_batch.h at dmxBatchSetFeedback has the definition).  The struct is
 * the caller's; a step fills it before it returns, for ball, hinge, slider and fixed joints and for contact joints created in the
 * near callback.  f1 / t1 belong to dJointGetBody(j, 0) and f2 / t2 to dJointGetBody(j, 1) -- after dJointAttach(j, 0, body) on an
 * articulation joint that is the body and the world; a side without a body reports zeros, a kinematic body its share.  A joint
 * that took no part in the step (a side destroyed, both sides the same) reports zeros.  Force or torque added by hand
 * (dJointAddHingeTorque, dJointAddSliderForce) is no part of it.  dJointSetFeedback(j, 0) forgets the struct; dJointDestroy and
 * dJointGroupEmpty do so too.  A world none of whose joints has a struct steps exactly as it does without this. */
typedef struct dJointFeedback { dVector3 f1, t1, f2, t2; } dJointFeedback;
void dJointSetFeedback(dJointID, dJointFeedback *);
dJointFeedback *dJointGetFeedback(dJointID);
int dAreConnected(dBodyID, dBodyID);
int dAreConnectedExcluding(dBodyID body1, dBodyID body2, int joint_type);

/* ---- rotation helpers used when filling dBodySetRotation's argument ------- */
void dRSetIdentity(dMatrix3 R);
void dRFromAxisAndAngle(dMatrix3 R, dReal ax, dReal ay, dReal az, dReal angle);
void dQtoR(const dQuaternion q, dMatrix3 R);
void dRtoQ(const dMatrix3 R, dQuaternion q);

/* ---- MI355X extension: bulk pose snapshot for the 60 Hz broadcast loop ------
 * (main.c:221-237 + GetTransformMat main.c:602-622): fills out[i*16 .. i*16+15]
 * (column-major 4x4) for bodies[i], i < n, in one device pass + one copy. */
int dmxWorldSnapshotTransforms(dWorldID, const dBodyID *bodies, int n, dReal *out);
/* The same over the reference's own arrays, in place of the loop main.c:221-237:
 *   dmxWorldSnapshotBodyStates(world, &bodies[0].body, sizeof(Body), MAX_BODIES,
 *                              bodyStates[0].transform, sizeof(BodyState));
 * handles that are 0 (empty slots and static geoms, main.c:228) are skipped, their states left as they are.
 * Returns the number of transforms written, -1 on error. */
int dmxWorldSnapshotBodyStates(dWorldID, const void *first_body, size_t body_stride, int n,
                               void *first_transform, size_t state_stride);

#ifdef __cplusplus
}
#endif
#endif
