/*
 * include/dmx_batch.h -- batch extension of the ODE-compatible C ABI.
 *
 * The reference drives ODE one geom pair at a time through a host callback
 * (dSpaceCollide -> NearCallback -> dCollide -> dJointCreateContact,
 * /root/reference/src/main.c:212, 674-693) and one body at a time through
 * dBodyCreate/dBodySet* (main.c:695-733) and dBodyGet* (main.c:221-237).
 * That shape cannot feed 10^6 bodies to a GPU, so the scenes of
 * BASELINE.json are driven through this batch form of the SAME calls: each
 * entry point below names the reference call (file:line) whose per-object
 * loop it replaces.  Plain C, plain pointers and sizes, no framework types.
 *
 * All state lives in HBM in one tiled slab (tiles of 64 bodies, see dmxBatchDevicePtr); `real` is float (DMX_F32,
 * ODE dSINGLE) or double (DMX_F64, ODE dDOUBLE) per batch.  Host arrays are
 * array-of-structs, row-major n x k, in the batch's precision.
 *
 * Every function returns 0 on success and a negative DMX_E* code on failure
 * (and prints the HIP error to stderr); nothing falls back to the CPU.
 */
#ifndef DMX_BATCH_H
#define DMX_BATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dmxBatch *dmxBatchID;

enum { DMX_F32 = 0, DMX_F64 = 1 };

enum {
    DMX_OK = 0,
    DMX_ENODEVICE = -1,   /* no usable HIP device */
    DMX_EHIP = -2,        /* a HIP call failed */
    DMX_EINVAL = -3,      /* bad argument */
    DMX_ENOMEM = -4,
    DMX_ECAPACITY = -5,   /* a fixed-size device table overflowed (broadphase bucket / pair buffer) */
    DMX_ECROSS = -6       /* two bodies owned by different ranks touch: the island has to be migrated to one owner */
};

/* per-body fields (k = components per body) */
enum {
    DMX_POS = 0,      /* k=3  dBodySetPosition / dBodyGetPosition   main.c:708, 229 */
    DMX_QUAT = 1,     /* k=4  (w,x,y,z); dBodySetRotation's R as q  main.c:709, 230 */
    DMX_LVEL = 2,     /* k=3  linear velocity  (0 at creation)      main.c:703      */
    DMX_AVEL = 3,     /* k=3  angular velocity (0 at creation)      main.c:703      */
    DMX_MASS = 4,     /* k=1  dBodySetMass mass  (default 1)             */
    DMX_INERTIA = 5,  /* k=3  body-frame principal inertia (default 1,1,1)          */
    DMX_SIDES = 6,    /* k=3  dCreateBox side lengths / (r,-,-) for a sphere  main.c:717,720 */
    DMX_FORCE = 7,    /* k=3  dBodyAddForce accumulator, cleared each step    main.c:532 */
    DMX_TORQUE = 8,   /* k=3  dBodyAddTorque accumulator                                  */
    DMX_QUAT_RAW = 9, /* k=4  like DMX_QUAT but stored as given (DMX_QUAT normalises on upload,
                              as dBodySetQuaternion does); for state that came from the device */
    DMX_STATE = 10,   /* k=13 pos3 quat4 lvel3 avel3 in one piece (the row layout of GatherBodies and of the boundary
                              pack): the whole read-back of main.c:221-237 in one transfer; the quaternion is stored
                              as given, like DMX_QUAT_RAW */
    DMX_NFIELDS = 11
};

/* geometry class per body (uint8 array) */
enum { DMX_GEOM_NONE = 0, DMX_GEOM_SPHERE = 1, DMX_GEOM_BOX = 2,     /* BodyType, inc/body.h:14-18 */
       DMX_GEOM_CONVEX = 3 };  /* a convex hull (BASELINE configs[4]); the reference itself creates none */

enum { DMX_GYRO_OFF = 0, DMX_GYRO_EXPLICIT = 1, DMX_GYRO_IMPLICIT = 2 };

/* dContactBounce etc: surface mode bits accepted by dmxBatchSetSurface */
enum { DMX_CONTACT_BOUNCE = 0x004 };
/* dContactApprox1_1 / _2 / both: friction that scales with the normal force -- see dmxContactJoint.  dmxBatchSetSurface accepts the
 * bits, but the ticks that find their own contacts (dmxBatchStep, dmxBatchStepTimed, dmxBatchStepRange, dmxBatchChunkTick(s),
 * dmxBatchExactTick) have not learnt them: while the batch surface would make a pyramid row (a bit set and 0 < mu < inf) they
 * return DMX_EINVAL, say why on stderr and leave the state untouched. */
enum { DMX_CONTACT_APPROX1_1 = 0x1000, DMX_CONTACT_APPROX1_2 = 0x2000, DMX_CONTACT_APPROX1 = 0x3000 };

/* ---- lifecycle: dInitODE/dWorldCreate/dHashSpaceCreate/dJointGroupCreate (main.c:94-98) */
int dmxDeviceCount(void);                 /* >=1 or DMX_ENODEVICE; never touches a CPU path */
/* (Creation also asks the HIP runtime for the attributes of every kernel a tick of this precision may launch: code objects and
 * per-kernel set-up load here, ~15 ms once per process and precision, rather than as a hitch at the first tick that needs the
 * exact pipeline -- DMX_PRELOAD=0 in the environment leaves that lazy.) */
int dmxBatchCreate(dmxBatchID *out, int64_t n_bodies, int precision, int device);
int dmxBatchDestroy(dmxBatchID b);        /* dWorldDestroy / dCloseODE  main.c:258-268 */
int64_t dmxBatchBodyCount(dmxBatchID b);
int dmxBatchPrecision(dmxBatchID b);

/* ---- world parameters */
int dmxBatchSetGravity(dmxBatchID b, double gx, double gy, double gz);      /* dWorldSetGravity main.c:96 */
int dmxBatchSetERP(dmxBatchID b, double erp);                                /* dWorldSetERP  (default 0.2) */
int dmxBatchSetCFM(dmxBatchID b, double cfm);                                /* dWorldSetCFM  (default 1e-5f / 1e-10) */
int dmxBatchSetQuickStep(dmxBatchID b, int iterations, double sor_w);        /* dWorldSetQuickStepNumIterations / W */
int dmxBatchSetGyroMode(dmxBatchID b, int mode);                             /* dBodySetGyroscopicMode + form */
/* NearCallback's per-contact surface, applied to every generated contact (main.c:684-687) */
int dmxBatchSetSurface(dmxBatchID b, int mode, double mu, double bounce, double bounce_vel);
int dmxBatchSetMaxContacts(dmxBatchID b, int max_contacts);                  /* dCollide flags (main.c:675,678) */
/* dCreatePlane(space,a,b,c,d): the one static half-space bodies collide with; enable=0 removes it */
int dmxBatchSetPlane(dmxBatchID b, double a, double bb, double c, double d, int enable);

/* AddBodyMap (main.c:735-761): n static, body-less box geoms -- the reference's floor and walls (main.c:115-121) --
 * created before every body, as the reference creates them: side lengths (n x 3), positions (n x 3) and rotations
 * (n x 12: the 3x4 row-major matrix dGeomSetRotation takes, main.c:749), doubles, rounded to the batch's precision.
 * Every body collides with every static box (the category / collide bits the reference ends up with, main.c:724-725,
 * 751-752); static boxes do not link dynamics islands and static-static pairs are ignored.  Contacts are dCollide(static
 * geom, body geom) in creation order: ground plane, static boxes in order, then body pairs.  n = 0 removes them;
 * at most DMX_MAX_STATIC_BOXES.
 * A body touching static geometry only (the ground plane, static boxes) is a dynamics island of its own; such bodies are
 * stepped by a fused path -- narrowphase against the plane and the static boxes, then rows + 20 sweeps + integration in
 * registers, one lane per body -- inside the same collision-proof chunks as free bodies (dmxBatchStep).  The path holds
 * 8 contacts per body (the reference's MAX_CONTACTS for ONE geom pair, main.c:675): a body with more (wedged between the
 * floor and two walls, say) sends its chunk through the exact path (pair search, narrowphase, island solve), which has no
 * such limit; with the collision proof switched off (dmxBatchSetBodyCollisions(b, 0)) nobody can, and such a body is
 * stepped with its first 8 contacts.  Same results as the exact path, bit for bit. */
#define DMX_MAX_STATIC_BOXES 64
int dmxBatchSetStaticBoxes(dmxBatchID b, int32_t n, const double *sides, const double *pos, const double *rot3x4);
/* dGeomSetCategoryBits / dGeomSetCollideBits (main.c:724-725, 751-752) at the granularity of geometry classes: whether bodies of
 * class_a and class_b (DMX_GEOM_SPHERE / BOX / CONVEX; symmetric) collide with one another.  Default: every class with every
 * class, as the reference's bits have it (CMASK_OBJ bodies collide with CMASK_OBJ | CMASK_MAP).  Pairs switched off are not kept
 * apart by the safe zones, not enumerated by the pair search and never reach a collider -- what ODE does with geoms whose bits do
 * not match.  (Static boxes and the ground plane collide with every body.) */
int dmxBatchSetClassPairs(dmxBatchID b, int class_a, int class_b, int enable);
/* DMX_STATIC_FUSED (default; DMX_STATIC_FAST=0 in the environment picks the other): as described above.  DMX_STATIC_EXACT:
 * every body whose bounding sphere reaches a static box goes through the exact path every tick (how round 2 did it; kept
 * for A/B runs and for the tests that hold the two against each other). */
enum { DMX_STATIC_EXACT = 0, DMX_STATIC_FUSED = 1 };
int dmxBatchSetStaticPath(dmxBatchID b, int mode);

/* ---- body data: replaces the AddBody loop (main.c:695-733) and the read-back loop (main.c:221-237) */
int dmxBatchUpload(dmxBatchID b, int field, const void *host_aos, int64_t first, int64_t count);
int dmxBatchDownload(dmxBatchID b, int field, void *host_aos, int64_t first, int64_t count);
int dmxBatchUploadGeomType(dmxBatchID b, const uint8_t *types, int64_t first, int64_t count);
/* dCreateConvex's point set for every DMX_GEOM_CONVEX body of the batch: n_points body-frame points (3 doubles each;
 * origin = centre of mass, e.g. from dmxHullBuild in dmx_hull.h).  *radius_out (may be NULL) = the hull's bounding
 * radius: upload it as sides[0] of every convex body (the broadphase reads it there, as it does a sphere's radius).
 * Contacts: convex against the ground plane as ODE's dCollideConvexPlane makes them (the hull's points in array order,
 * the first max_contacts <= 8 on or below the plane); against boxes, spheres and other convex bodies: this library's own
 * colliders, which need the hull's faces (dmxBatchSetConvexHullFaces below). */
int dmxBatchSetConvexHull(dmxBatchID b, int32_t n_points, const double *points_xyz, double *radius_out);
/* dCreateConvex's plane set for the same hull: n_faces x 4 doubles (unit outward normal, offset; body frame), e.g. from
 * dmxHullPlanes.  Contacts of a convex body with BOXES -- static boxes (dmxBatchSetStaticBoxes: the floor of BASELINE
 * configs[4]) and box bodies -- are this library's own collider (ODE's dCollideConvexBox is an empty stub): hull vertices
 * inside the box in array order, each along the box face it is nearest to, then -- with the faces given here -- box
 * corners inside the hull, each along the hull face it is nearest to; the first max_contacts <= 8 are kept (edge-edge
 * penetrations are not detected).  Convex against CONVEX (both bodies carry the batch's one hull): the same two primitives --
 * the second body's vertices inside the first, in array order, each along the first's face it is nearest to, then the first
 * body's vertices inside the second; the first max_contacts are kept.  SPHERE against convex: the hull's face planes' largest
 * signed distance to the sphere's centre (first face on ties); within the radius, one contact along that face -- exact over a
 * face's interior, met early by up to (1 - cos) of the radius over an edge or a vertex.  Without the faces a convex body
 * collides with the ground plane only. */
int dmxBatchSetConvexHullFaces(dmxBatchID b, int32_t n_faces, const double *planes);
/* device address of component c of a field for body 0.  The slab is tiled: bodies are stored in tiles of
 * DMX_SLAB_TILE; inside a tile each of the DMX_SLAB_COMPONENTS components holds DMX_SLAB_TILE consecutive
 * reals, so body i's value sits (i / DMX_SLAB_TILE) * DMX_SLAB_COMPONENTS * DMX_SLAB_TILE + i % DMX_SLAB_TILE
 * reals after the returned address.  dmxBatchStride = bodies the slab is allocated for (a multiple of 256).
 * The batch keeps TWO slabs of this layout and the state alternates between them (see dmxBatchSetSnapshotMode): the
 * address is that of the slab holding the current state and is valid until the next step / chunk call. */
#define DMX_SLAB_TILE       64
#define DMX_SLAB_COMPONENTS 30
void *dmxBatchDevicePtr(dmxBatchID b, int field, int component);
int64_t dmxBatchStride(dmxBatchID b);

/* ---- stepping: the tick loop of main.c:211-215 (collide -> step -> clear contacts), nsteps times.
 * Asynchronous on the batch's stream.  QuickStep semantics. */
int dmxBatchStep(dmxBatchID b, double h, int nsteps);
int dmxBatchSynchronize(dmxBatchID b);
/* Island sharding across GPUs: slots [0, n_active) are this rank's own bodies and are stepped;
 * slots [n_active, n) hold read-only ghost copies of neighbouring ranks' boundary bodies.  n_active must be
 * a multiple of 4 (or n).  dmxBatchStepRange steps one tick over [first, first+count) only, so boundary
 * rows can be stepped (and sent) before the interior; first/count must be multiples of 16 B / sizeof(real). */
int dmxBatchSetActiveCount(dmxBatchID b, int64_t n_active);
/* boundary-row pack fused into the step kernels: every whole-slab tick also writes the new 13-real state of bodies
 * [0, lo_count) and [hi_first, n_active) to out_dev (AoS, lower rows first), ready for the all-gather; NULL = off */
int dmxBatchSetBoundaryPack(dmxBatchID b, void *out_dev, int64_t lo_count, int64_t hi_first);
int dmxBatchStepRange(dmxBatchID b, double h, int64_t first, int64_t count, int reset_diag);
/* run on a caller-owned hipStream_t (e.g. the framework's current stream); NULL restores the batch's own */
int dmxBatchSetStream(dmxBatchID b, void *hip_stream);
int dmxBatchGetStream(dmxBatchID b, void **hip_stream);
/* step nsteps times bracketed by HIP events on the batch's stream; *ms = elapsed device milliseconds */
int dmxBatchStepTimed(dmxBatchID b, double h, int nsteps, float *ms);

/* ---- body-body collisions inside dmxBatchStep (dSpaceCollide for body pairs, main.c:212).
 * enable = 1 (default): every tick proves the body-pair set empty through per-body broadphase safe zones, or,
 * when a body leaves its zone / bodies are crowded, runs the exact pair search + narrowphase + island solve
 * for the bodies involved; results equal the sequential oracle's either way.  enable = 0: the caller asserts
 * that bodies never touch one another (every island is a single body) and the check is skipped.
 * stats: [0] ticks in fast mode, [1] ticks in exact mode, [2] safe-zone rebuilds, [3] ticks that had body
 * pairs, [4] body pairs in the last tick, [5] crowded bodies at the last rebuild. */
int dmxBatchSetBodyCollisions(dmxBatchID b, int enable);
/* How a collision-proof chunk keeps its start state for a rollback.
 * DMX_SNAPSHOT_PINGPONG (default): the batch owns two slabs; the chunk's first launch reads one and writes the new state
 * to the other, later launches run in place there, a rollback swaps back -- no copy, no extra HBM traffic.
 * DMX_SNAPSHOT_COPY: the 13 state components are copied aside at the chunk's start and the state never changes slab --
 * for callers that replay captured HIP graphs of ticks, which bake the slab's address in.  Not inside a chunk. */
enum { DMX_SNAPSHOT_PINGPONG = 0, DMX_SNAPSHOT_COPY = 1 };
int dmxBatchSetSnapshotMode(dmxBatchID b, int mode);
/* How an exact tick (bodies in pairs / at static boxes) runs its bookkeeping -- pair list, islands, joints by island, level
 * schedules.  STAGED: a launch per stage over as many compute units as the stage fills.  ONE_WORKGROUP: the same stages, in
 * the same order, inside two one-workgroup kernels around the narrowphase (barriers instead of ~25 launches), whenever the
 * tick's arrays fit one workgroup (<= 8192 slots and entries); AUTO (default; DMX_SMALL_EXACT=0/2 in the environment picks
 * one of the others): ONE_WORKGROUP for scenes of up to 2048 slots whose last tick had at most 512 pairs.  Same results,
 * bit for bit, either way. */
enum { DMX_EXACT_AUTO = 0, DMX_EXACT_STAGED = 1, DMX_EXACT_ONE_WORKGROUP = 2 };
int dmxBatchSetExactPipeline(dmxBatchID b, int mode);
/* Contact-free ticks (no ground plane) may be taken `ticks` at a time inside one kernel launch, the bodies' state held
 * in registers between them: same arithmetic per tick, same results bit for bit, one read and one write of the state
 * per launch instead of per tick.  Default 1 (one launch per tick); 1..64. */
int dmxBatchSetTicksPerLaunch(dmxBatchID b, int ticks);
/* Work the contact-free tick (integrate_free) leaves out because the result does not need it; same results bit for bit
 * with any mask.  DMX_ELIDE_STORES: a launch that runs in place stores a state component of a wavefront's 64 bodies only
 * if one of them changed its bits (a body dropped at rest under gravity along y keeps lvel.x/z, pos.x/z and, with isotropic
 * inertia, avel).  DMX_ELIDE_CONSTANTS: while every slot's mass and inertia are the same -- the library follows the uploads
 * of DMX_MASS / DMX_INERTIA; any dmxBatchDevicePtr call ends it for the batch's lifetime (the address is one into the slab,
 * through which the caller can write every component unseen) -- they are passed as kernel arguments instead of loaded per
 * body.  Launches recorded while the batch's stream is being captured into a HIP graph always load them, so that a replay
 * sees a later upload of mass or inertia like an eager tick does.  Default: both (DMX_ELIDE=<mask> in the environment changes the default); 0: every load and store. */
enum { DMX_ELIDE_STORES = 1, DMX_ELIDE_CONSTANTS = 2 };
int dmxBatchSetElision(dmxBatchID b, int mask);
/* A third removal, active only while DMX_ELIDE_STORES is on: loads of lateral state a tile has proven fixed.  The library keeps
 * one word per 64-body tile on the device; an axis k of a tile is fixed once a launch has loaded pos.k and lvel.k of the tile's
 * bodies, run the tick and found the bits of both unchanged in every lane -- the tick computes them from themselves, h, g.k and
 * the mass, so the same launch again would find the same.  One-tick launches over the whole active slab then leave out the
 * loads, ballots and stores of pos.x/lvel.x and pos.z/lvel.z in such tiles (13 -> 9 state loads for bodies dropped at rest under
 * gravity along y), for as long as nothing but such launches with the same h, gravity, mass, gyro mode, active count and elision
 * mask touches the batch: any other call of this API than dmxBatchStep / dmxBatchChunkTick(s) themselves, a rollback, an exact or
 * joints tick makes the next launch load everything and establish the words anew (csrc/dmx_fixed.hpp has the rule).  Any
 * dmxBatchDevicePtr call, and any stepping call made while the batch's stream is being captured into a HIP graph, end it for the
 * batch's lifetime.  Same results bit for bit.  Default on (DMX_ELIDE_LOADS=0 in the environment, read at dmxBatchCreate: off). */
int dmxBatchSetLoadElision(dmxBatchID b, int on);
/* Arithmetic the contact-free tick does not need: a body whose torque is exactly zero -- no force accumulators in the launch, no
 * gyroscopic torque (gyro mode 0, or an isotropic inertia) -- gets w += Iw^-1 (h * 0) = w + (+0) from the general tick, so a launch
 * whose mass and inertia are uniform (DMX_ELIDE_CONSTANTS active), whose h is finite and positive and whose every 1/I.k is finite
 * and at most the largest finite number / 1024 steps a wavefront with the short tick, which builds neither the rotation matrix nor
 * the world-frame inverse inertia, whenever every lane's quaternion has |q.k| <= 2; any other wavefront runs the general tick in the
 * same kernel (csrc/dmx_torque_free.hpp has the rule).  Same results bit for bit.  Default on (DMX_TORQUE_FREE=0 in the
 * environment, read at dmxBatchCreate: off -- the launches are then the ones they always were). */
int dmxBatchSetTorqueFree(dmxBatchID b, int on);
/* for tests and diagnostics: [0] contact-free launches so far that took a kernel with the short tick built in (the rule said on),
 * [1] those that took the general kernel.  Which wavefronts of a launch pass the quaternion guard is not counted. */
int dmxBatchTorqueFreeStats(dmxBatchID b, int64_t out[2]);
/* Instructions the lean launch does not need: a contact-free launch that is lean (dmxBatchSetLoadElision), has its constants as
 * arguments and takes the short tick (dmxBatchSetTorqueFree) -- one tick, in place, no force accumulators -- runs a kernel of its
 * own whose wavefronts read a compact argument block, step one tile in a straight line when the tile's lateral axes are fixed and
 * every quaternion passes the short tick's guard, and run the general launch's tile body otherwise.  Same results bit for bit.
 * Default on (DMX_LEAN_KERNEL=0 in the environment, read at dmxBatchCreate: off -- the launches are then the ones they always were). */
int dmxBatchSetLeanKernel(dmxBatchID b, int on);
/* for tests and diagnostics: [0] contact-free launches so far that took that kernel, [1] those that did not */
int dmxBatchLeanKernelStats(dmxBatchID b, int64_t out[2]);
/* for tests and diagnostics, never on a hot path (takes the counts, then settles the batch -- which, like every observer, breaks
 * the chain: that break shows in the next call's count -- and reads the words back): [0] launches that established the
 * words, [1] lean launches, [2] times the chain was broken, [3] 1 once ended for good, [4] / [5] tiles of the active range whose
 * word says x / z fixed, as the last establishing or lean launch left them */
int dmxBatchLoadElisionStats(dmxBatchID b, int64_t out[6]);
int dmxBatchCollisionStats(dmxBatchID b, int64_t out[6]);
/* the same six numbers and [6] AABB pairs met so far that had no collider (always 0 since every class pair has one), [7] exact ticks
 * of the one-workgroup pipeline whose island solve and fused step were enqueued before the host had the tick's counts, and stood
 * (the device's record gates them; DMX_SPECULATE=0 in the environment makes every tick wait for its counts first) */
int dmxBatchCollisionStatsEx(dmxBatchID b, int64_t out[8]);

/* ---- the collision-checked tick loop in pieces.  dmxBatchStep(b, h, n) with body collisions enabled runs, inside
 * the library: [zones, snapshot] -> k checked ticks -> one flag read -> commit, or roll back and replay exactly.  A
 * caller that has work of its own between ticks -- the multi-GPU boundary exchange, which refreshes the ghost slots
 * [active count, body count) every tick -- drives the same steps itself:
 *   ChunkBegin   rebuild stale safe zones (ghost slots included), arm the rollback snapshot (dmxBatchSetSnapshotMode),
 *                clear the violation flag;
 *                *exact_only = 1 when the fast path may not be used (crowded bodies, pending external forces),
 *                *ballistic = 1 when bodies move on straight horizontal lines, so checking the chunk's first
 *                and last tick proves the ticks between
 *   ChunkTick    one fused tick of the active bodies, with or without the safe-zone check.  A checked tick of a scene with
 *                a ground plane does nothing once the violation flag is up (the chunk will be rolled back whole: the
 *                only thing a caller may do after a violation)
 *   CheckZonesOnStream  the check alone for slots [first, first+count), on the caller's stream (ghost slots after
 *                their refresh)
 *   RefreshGhostsOnStream  the per-tick ghost refresh in one launch on the caller's stream: the lower neighbour's rows
 *                (13 reals per body, as GatherBodies / the boundary pack lay them out) into slots [first,
 *                first+count_lo), the upper neighbour's into the count_hi slots behind; a NULL source leaves its
 *                range untouched; check = 1 also tests the new positions against the slots' zones
 *   ChunkEnd     wait for the batch stream and report the flags; the caller combines them over ranks
 *   ChunkCommit  account `ticks` fast ticks; refresh_zones = 1 schedules a zone rebuild (the warn flag was up)
 *   ChunkRollback  restore the state the chunk's first tick started from, ghost slots included (zones are rebuilt at the
 *                next ChunkBegin).  Whatever writes state between ticks (the ghost refresh) does so after that tick
 *   ExactTick    one tick with the exact pair search / narrowphase / island solve; DMX_ECROSS if a pair involves
 *                a ghost slot */
int dmxBatchChunkBegin(dmxBatchID b, int *exact_only, int *ballistic);
int dmxBatchChunkTick(dmxBatchID b, double h, int check);
/* n ticks of a ballistic chunk: the test at the run's first / last tick only, as asked */
int dmxBatchChunkTicks(dmxBatchID b, double h, int nticks, int check_first, int check_last);
int dmxBatchCheckZonesOnStream(dmxBatchID b, void *hip_stream, int64_t first, int64_t count);
int dmxBatchRefreshGhostsOnStream(dmxBatchID b, void *hip_stream, int64_t first, int64_t count_lo, const void *src_lo,
                                  int64_t count_hi, const void *src_hi, int check);
int dmxBatchChunkEnd(dmxBatchID b, int *violated, int *warn);
int dmxBatchChunkCommit(dmxBatchID b, int ticks, int refresh_zones);
int dmxBatchChunkRollback(dmxBatchID b);
int dmxBatchExactTick(dmxBatchID b, double h);

/* ---- dSpaceCollide's pair search alone (main.c:212), for the callback form of the tick: the device finds every pair of
 * bodies (i < j, ascending i then j) whose geoms' AABBs overlap, and the bodies "involved" -- in such a pair, or with
 * their AABB overlapping a static box's (dmxBatchSetStaticBoxes) -- ascending.  The arrays are host memory owned by the
 * batch, valid until its next call.  The ODE API face (dSpaceCollide in libode_mi355) feeds the user's near callback from
 * this list when the world is large enough for the device search to pay. */
int dmxBatchFindPairs(dmxBatchID b, const int32_t **pairs, int64_t *n_pairs, const int32_t **involved, int64_t *n_involved);
/* Island sharding: the (own body, ghost slot) pairs the last dmxBatchFindPairs met -- bodies of this rank whose
 * AABB overlaps a neighbouring rank's boundary body.  Their island spans two ranks; the host loop migrates it to one owner
 * (rl-ode-physics_amd/shard.py) before the exact tick, which would otherwise return DMX_ECROSS.  At most 256 are listed. */
int dmxBatchCrossPairs(dmxBatchID b, const int32_t **pairs, int64_t *n_pairs);

/* ---- ray casts: the scene query ODE answers with a ray geom (dCreateRay + dCollide), in batch form.  Each ray is the segment
 * origin + t * dir, 0 <= t <= length, dir normalised in the batch's precision (7 reals: origin3 dir3 length); it reports the
 * FIRST geom whose surface it crosses: a body slot, the ground plane (dmxBatchSetPlane) or a static box (dmxBatchSetStaticBoxes).
 *   ids[i]   the body's slot (>= 0), DMX_RAY_MISS, DMX_RAY_PLANE, or DMX_RAY_STATIC_BOX(k) = -3 - k for static box k
 *   hits[i]  7 reals in dContactGeom's order: pos3, normal3, depth = t.  The normal is the surface's outward unit normal at the
 *            hit, negated when the origin lies inside the solid: dot(normal, dir) <= 0 (what ODE's ray colliders return).  A
 *            miss gives the segment's end point, a zero normal and depth = length; a ray whose direction has zero or non-finite
 *            norm, or whose length is non-finite or <= 0, gives DMX_RAY_MISS and seven zeros.
 * Equal t: the plane wins, then static boxes in order, then bodies by slot -- the answer never depends on the search order.
 * Visible: every slot of [0, body count), ghost slots included, whose class is not DMX_GEOM_NONE, whose flags have
 * DMX_BODY_ALIVE and whose class bit is in `mask`.  Convex bodies are seen through the hull's faces
 * (dmxBatchSetConvexHullFaces): without faces a convex body is invisible to rays, as it collides with the ground plane only.
 * Rays see the state after every tick enqueued so far: a cast first settles the chunk dmxBatchStep may have left open, like every
 * call that observes the batch.  Beyond that it changes nothing a later tick can tell: the same states with and without casts
 * between the ticks, and the same statistics as with a dmxBatchSynchronize in each cast's place.
 * dmxBatchRayCast takes and fills host arrays and returns when they are filled.  dmxBatchRayCastDevice takes device pointers
 * and is enqueued on the batch's stream; it waits for the device only when the column grid the rays walk has to be rebuilt,
 * which happens at the first cast after the state, the extents, the classes or the flags changed (many casts between two
 * ticks share one build; a batch whose slab address was handed out by dmxBatchDevicePtr rebuilds at every cast).
 * Three forms of the same computation, same results bit for bit: a lane per ray walking the hashed (x,z) column grid (above
 * 4 096 rays), a wavefront per ray (up to 4 096 rays: one pick ray into a crowded pen), and a brute-force form that tests
 * every slot (never chosen automatically; the cross-check).  dmxBatchSetRayForm, or DMX_RAY_FORM=lane|wave|brute in the
 * environment (the setter wins), forces one. */
enum { DMX_RAY_MISS = -1, DMX_RAY_PLANE = -2 };
#define DMX_RAY_STATIC_BOX(k) (-3 - (k))
enum { DMX_RAY_SPHERES = 1, DMX_RAY_BOXES = 2, DMX_RAY_CONVEX = 4, DMX_RAY_STATIC = 8, DMX_RAY_PLANE_BIT = 16, DMX_RAY_ALL = 31 };
enum { DMX_RAY_FORM_AUTO = 0, DMX_RAY_FORM_LANE = 1, DMX_RAY_FORM_WAVE = 2, DMX_RAY_FORM_BRUTE = 3 };
int dmxBatchRayCast(dmxBatchID b, int64_t n_rays, const void *rays_aos, int32_t *ids, void *hits_aos, uint32_t mask);
int dmxBatchRayCastDevice(dmxBatchID b, int64_t n_rays, const void *rays_dev, int32_t *ids_dev, void *hits_dev, uint32_t mask);
int dmxBatchSetRayForm(dmxBatchID b, int form);

/* ---- explicit contact joints: the callback form of the tick.  The reference's near callback makes one
 * dJointCreateContact + dJointAttach per contact (main.c:683-692) and then calls dWorldStep (main.c:213);
 * this entry takes the whole tick's contact joints at once, groups them into dynamics islands, and steps
 * every live body (bodies without joints integrate freely).  body2 = -1 (or body1 = -1) means static
 * geometry (dGeomGetBody == 0, main.c:691); the normal points into body1 as dCollide returns it. */
typedef struct dmxContactJoint {
    double pos[3], normal[3], depth;      /* dContactGeom */
    int32_t body1, body2;                 /* body slots, -1 = none */
    int32_t mode;                         /* dContactBounce | dContactSoftERP | dContactSoftCFM | DMX_CONTACT_APPROX1_1 / _2 (below) */
    double mu, bounce, bounce_vel, soft_erp, soft_cfm;   /* dSurfaceParameters (main.c:684-687) */
} dmxContactJoint;
/* Friction (dContactApprox1).  By default a contact's friction rows are box-bounded, lo = -mu, hi = +mu: mu is a FORCE, ODE's
 * default.  Friction row d (1 or 2) of a contact joint is a PYRAMID ROW when bit DMX_CONTACT_APPROX1_d of its mode is set and
 * 0 < mu < +inf: its bound is mu times the contact's normal force, and mu is the friction coefficient.  Every other row is what it
 * is without the bits: mu = +inf with a bit set is the unbounded row (ODE's |inf * 0| would be NaN), mu <= 0 still makes one row.
 * Row count, row order (creation order, a contact's friction rows directly behind its normal row), island building and the set of
 * rows that can never clamp depend on mu alone, not on the bits.  ODE's dContactApprox1_N (0x4000, rolling friction) has no meaning:
 * there are no rolling rows.  dContactMu2, dContactFDir1, dContactMotion* and dContactSlip* have no field here and are ignored by
 * dmxBatchStepJoints: they travel in dmxContactSurface, through dmxBatchStepJointsSurface (below), which makes mu a per-row mu_r.
 *   QuickStep (DMX_STEPPER_QUICK, DMX_ORDER_CREATION): when a sweep visits a pyramid row, hi = |mu lambda_n|, lo = -hi, lambda_n = the
 *     CURRENT multiplier of the contact's normal row, already updated in this sweep (ODE's SOR_LCP); nothing else about the update
 *     changes.  ODE moves such rows to the end of its row order; this library keeps creation order.  Under DMX_ORDER_ODE with
 *     QuickStep a tick with a pyramid row returns DMX_EINVAL (one line on stderr, the state untouched), as with articulation joints.
 *   dWorldStep (DMX_STEPPER_EXACT): this library's definition -- an island with a pyramid row is solved twice: pass A is the box LCP
 *     with every pyramid row held at lo = hi = 0 and yields lambda^A; pass B is the box LCP with the pyramid rows bounded by
 *     -/+ mu lambda^A_n and yields the lambda the tick and the feedback use.  (What ODE's Dantzig solver does for the first friction
 *     row it adds -- the bound from the normal force of the friction-free solution -- made independent of the row order.)  Both
 *     passes are positive definite box LCPs with unique solutions.  An island without a pyramid row is solved once, as before.
 *   Feedback (dmxBatchContactFeedback) is J^T lambda of the final lambda.
 *   The single-launch tick honours pyramid rows under QuickStep; under dWorldStep a tick with a pyramid row takes the general path,
 *   whole, and counts under DMX_SMALL_TICK_STAT_LDS_FIT. */
int dmxBatchStepJoints(dmxBatchID b, double h, int64_t n_joints, const dmxContactJoint *joints);
/* The rest of ODE's contact surface (dContactMu2, dContactFDir1, dContactMotion1 / 2 / N, dContactSlip1 / 2).  dmxContactJoint is ABI
 * and has no spare field, so the seven fields travel beside it: surfaces[k] belongs to joints[k], and bit X of joints[k].mode says
 * that field X of surfaces[k] is read.  Fields without their bit are never read.  The values of the bits are ODE's.
 *   surfaces == NULL is dmxBatchStepJoints, call for call; and dmxBatchStepJoints itself goes on ignoring the seven bits.
 *   A tick is an EXTENDED TICK when some contact that survives canonicalisation and the auto-disable drop has a bit of
 *   DMX_CONTACT_SURFACE_EXT set.  A tick with surfaces != NULL that is not extended stages, launches and loads exactly what
 *   dmxBatchStepJoints does; an extended tick launches the kernels a tick with a pyramid row launches (DMX_CONTACT_APPROX1).
 * This library's definition ([ODE-recall] where it follows ODE's dxJointContact::getInfo2):
 *   Coefficients.  mu_1 = max(mu, 0); mu_2 = max(surface.mu2, 0) with MU2, else mu_1.  The contact has three rows when
 *     max(mu_1, mu_2) > 0, else one.  [ODE-recall] ODE leaves out a friction row whose coefficient is 0; this library keeps three
 *     rows per contact and builds that row with lo = hi = 0: its multiplier is 0 under both steppers, the velocities are the same.
 *   Sides.  Canonicalisation is dmxBatchStepJoints': when body1 is not a live slot the sides are exchanged and the normal negated;
 *     n is the canonical normal.
 *   Directions.  Row 0 is along n.  With FDIR1: d_1 = fdir1 as given, d_2 = n x d_1 [ODE-recall]; fdir1 is neither normalised nor
 *     projected -- unit length and orthogonality to the normal are the caller's duty, as in ODE.  Without: dPlaneSpace(n), as before.
 *   Bounds of friction row r (1 or 2) with coefficient mu_r: 0 gives lo = hi = 0; +inf the unbounded row, whatever the Approx1 bit;
 *     otherwise a pyramid row with coefficient mu_r when DMX_CONTACT_APPROX1_r is set, else the box row -/+ mu_r.  dWorldStep's
 *     two passes and QuickStep's moving bound (above) apply with mu_r in place of mu.
 *   Right-hand side.  Row 0: c = erp / h * max(depth - surface_layer, 0) + (MOTIONN ? motionN : 0), then the max_correcting_vel cap,
 *     then the bounce rule.  Row 1: c = MOTION1 ? motion1 : 0.  Row 2: c = MOTION2 ? motion2 : 0.  The meaning, in CANONICAL
 *     sides: (v_p1 - v_p2) . d_r = c_r, v_pi = the velocity of body i's material point at pos (0 for the world), body 1 the live
 *     body the canonical normal points into, d_2 = n x d_1.  No motion changes sign where the sides were exchanged, whatever made
 *     d_1: a body on a belt (the world, fdir1 along the belt, motion1 = u) is carried along +fdir1 at u whether the joint was
 *     given as (body, world) or as (world, body).  That keeps a belt's direction independent of the order of the two bodies (of
 *     dJointAttach's arguments); what stock ODE does on this point is not checked.
 *   Slip.  Row r's CFM is slip_r with SLIPr, else the world's CFM.  It is divided by h like every row's; the multiplier is a force,
 *     so the row slides at slip_r times its friction force [ODE-recall].
 *   Refused with DMX_EINVAL, one line on stderr, the state and the last tick's feedback untouched: a read field of any joint given
 *     that is NaN; a read slip that is negative or not finite; a read motion or fdir1 component that is not finite -- each judged
 *     as the batch will hold it: in a DMX_F32 batch a double above float's largest is an infinity; an extended tick under
 *     DMX_ORDER_ODE with QuickStep.  (mu and mu2 are likewise taken rounded to the batch's precision when rows are counted.)  Bits of
 *     the mode above ODE's (0x10000 and up) mean nothing and are not passed on.  (A tick of a subset of the bodies cannot receive surfaces: the ticks that find
 *     their own contacts do not come through here.)
 *   The one-body forms know box friction only: an extended tick's one-body islands take the row form.  The single-launch tick
 *   honours an extended QuickStep tick; an extended dWorldStep tick takes the general path, whole, and counts under
 *   DMX_SMALL_TICK_STAT_LDS_FIT.  Feedback, auto-disable and damping work as in every dmxBatchStepJoints tick. */
enum { DMX_CONTACT_MU2 = 0x001, DMX_CONTACT_FDIR1 = 0x002, DMX_CONTACT_MOTION1 = 0x020, DMX_CONTACT_MOTION2 = 0x040,
       DMX_CONTACT_MOTIONN = 0x080, DMX_CONTACT_SLIP1 = 0x100, DMX_CONTACT_SLIP2 = 0x200, DMX_CONTACT_SURFACE_EXT = 0x3e3 };
typedef struct dmxContactSurface { double mu2, fdir1[3], motion1, motion2, motionN, slip1, slip2; } dmxContactSurface;  /* 72 bytes */
int dmxBatchStepJointsSurface(dmxBatchID b, double h, int64_t n_joints, const dmxContactJoint *joints, const dmxContactSurface *surfaces);
/* Which of ODE's two steppers dmxBatchStepJoints is.  DMX_STEPPER_QUICK (default): dWorldQuickStep, QuickStep's SOR sweeps.
 * DMX_STEPPER_EXACT: dWorldStep, the reference's own call (main.c:213): every island's system
 *   A lambda = b + w,  A = J M^-1 J^T + cfm / h,  lo <= lambda <= hi,  w complementary to lambda
 * -- the same contact rows -- is solved exactly (block principal pivoting over a Cholesky of the free block; A is positive
 * definite, so the solution is the one ODE's Dantzig solver reaches): small islands one workgroup each, islands of
 * DMX_LCP_GRID_ROWS (192) rows or more -- the reference's pen holds up to 512 bodies in one island of 2 000 - 2 600 rows
 * (main.c:208,213, inc/body.h:6) -- by a grid-wide blocked factorisation on the matrix cores with the rows that can never
 * clamp eliminated once per tick and the active set carried from tick to tick (csrc/dmx_lcp.hip).  Cost grows with the cube
 * of an island's rows, as dWorldStep's does; a tick with an island above DMX_MAX_EXACT_ROWS (16 384) rows is stepped with
 * the SOR instead (stderr says so).  dmxBatchStep (the BASELINE configs, which name dWorldQuickStep) is not affected. */
enum { DMX_STEPPER_QUICK = 0, DMX_STEPPER_EXACT = 1 };
int dmxBatchSetStepper(dmxBatchID b, int stepper);
/* Counters of the grid-wide exact solve since the batch was created: out[0] island solves, [1] pivoting rounds in all,
 * [2] most rounds in one solve, [3..5] rows / never-clamping rows / bounded rows of the last island solved, [6] rounds that
 * flipped a single row (Murty's rule), [7] ticks stepped with the SOR because an island exceeded DMX_MAX_EXACT_ROWS. */
int dmxBatchLcpStats(dmxBatchID b, int64_t out[8]);
/* The single-launch tick of small worlds (csrc/dmx_small.hip).  A dmxBatchStepJoints tick of a world of tens of bodies is
 * bound by launches and copies, not arithmetic; when the tick is ELIGIBLE it runs as one kernel launch with no copy in either
 * direction: the tick's tables are read from host-mapped pinned staging, and every body's 13 state reals are written to the
 * slab and to a host-mapped mirror that dmxBatchDownload(DMX_STATE) serves from after waiting for the tick.  Eligible: mode
 * AUTO; rows in creation order (not DMX_ORDER_ODE under QuickStep); the whole batch stepped from host contact geometry; at
 * most 512 live bodies (in a batch of at most 4 096 slots) and 512 islands; QuickStep: no island of more than 256 rows;
 * dWorldStep: every island's solve fits one workgroup's LDS.  Any other tick runs on the general path, whole: same results
 * (the kernels share their device functions), no mixed ticks.  DMX_SMALL_TICK=0 in the environment makes OFF the default of
 * every batch of the process; DMX_SMALL_TICK_REPORT=1 prints the counters to stderr when a batch is destroyed. */
#define DMX_SMALL_TICK_OFF   0   /* never */
#define DMX_SMALL_TICK_AUTO  1   /* default: when the tick is eligible */
int dmxBatchSetSmallTick(dmxBatchID b, int mode);
/* Counters since the batch was created: ticks on the single-launch path, ticks of dmxBatchStepJoints on the general path,
 * then per reason the ticks that were not eligible (a tick counts under the first reason that applies, in this order).
 * DMX_SMALL_TICK_STAT_LDS_FIT also counts the dWorldStep ticks that have a pyramid row (DMX_CONTACT_APPROX1) -- their two passes are
 * the general path's -- and the extended dWorldStep ticks of dmxBatchStepJointsSurface. */
enum {
    DMX_SMALL_TICK_STAT_SMALL = 0, DMX_SMALL_TICK_STAT_GENERAL = 1, DMX_SMALL_TICK_STAT_MODE = 2, DMX_SMALL_TICK_STAT_ROW_ORDER = 3,
    DMX_SMALL_TICK_STAT_SUBSET = 4, DMX_SMALL_TICK_STAT_BODIES = 5, DMX_SMALL_TICK_STAT_ISLANDS = 6, DMX_SMALL_TICK_STAT_SOR_ROWS = 7,
    DMX_SMALL_TICK_STAT_LDS_FIT = 8
};
#define DMX_SMALL_TICK_NSTATS 9
int dmxBatchSmallTickStats(dmxBatchID b, int64_t out[DMX_SMALL_TICK_NSTATS]);
/* The order QuickStep's SOR sweeps an island's rows in (dmxBatchStepJoints, DMX_STEPPER_QUICK).  DMX_ORDER_CREATION (default):
 * the order the contact joints were created in, every sweep -- deterministic, and what lets islands be solved by workgroups
 * under a level schedule.  DMX_ORDER_ODE: what stock ODE does [ODE-recall]: rows numbered in the order its island builder
 * discovers the joints (depth-first from the newest body, each body's joints newest first) and re-shuffled before sweeps
 * 0, 8, 16, ... with ODE's linear congruential generator (RANDOMLY_REORDER_CONSTRAINTS), seeded here per batch (`seed` =
 * dRandSetSeed; ODE's generator is process-global).  Islands are then swept sequentially, one lane each: an option for
 * comparing with ODE's own sequence, not a fast path.  "Newest body" is the highest slot. */
enum { DMX_ORDER_CREATION = 0, DMX_ORDER_ODE = 1 };
int dmxBatchSetRowOrder(dmxBatchID b, int order, uint32_t seed);

/* ---- articulation joints: ball-and-socket and hinge (dJointCreateBall / dJointCreateHinge); slider and fixed, and angular motors: further below.  Unlike contact joints, which
 * live for one tick, the set given to dmxBatchSetJoints persists until it is replaced and takes part in every
 * dmxBatchStepJoints tick -- both steppers, both precisions, the general path and the single-launch tick of small worlds.
 * Anchors and axes are stored in the frames of the two bodies (world frame for a side that is -1, the world).
 *   active       a joint is inactive for a tick when both sides are -1, when both sides are the same slot, or when a side that
 *                is >= 0 is not alive.  body1 = -1 with a live body2 exchanges the two sides (anchors and axes included).  A
 *                kinematic body is a side like any other (its inverse mass is zero).
 *   row order    within an island the active articulation joints come first, in the order of the set, then the tick's contact
 *                joints in creation order; articulation joints link islands as contact joints between two bodies do.
 *   rows         x_i, R_i = body i's position and rotation, a_i = R_i anchor_i (a world side: x = anchor, a = 0, no Jacobian
 *                block); every row has lo = -inf, hi = +inf, cfm = the world's CFM; k = ERP / h.  (A hinge's limit / motor row,
 *                the one row of a joint that can clamp: dmxBatchSetHingeLimots below.)
 *                ball:  three rows, d = e_x, e_y, e_z:  J = [ d, a_1 x d | -d, -(a_2 x d) ],  c = k ((x_2 + a_2) - (x_1 + a_1)) . d
 *                hinge: the three ball rows, then with u = R_1 axis1, w = R_2 axis2, (p, q) = dPlaneSpace(u), for r = p, q:
 *                       J = [ 0, r | 0, -r ],  c = k (u x w) . r
 * While a non-empty set is present, the ticks that find their own contacts and build islands on the device -- dmxBatchStep,
 * dmxBatchStepTimed, dmxBatchStepRange, dmxBatchChunkTick(s), dmxBatchExactTick -- and QuickStep's dmxBatchStepJoints under DMX_ORDER_ODE
 * return DMX_EINVAL with one line on stderr: nothing is silently ignored.  (Under DMX_STEPPER_EXACT the row order is never used, so
 * there is nothing to refuse.)  Everything else is unaffected; dmxBatchLastContactCount goes on counting contact joints only. */
enum { DMX_JOINT_BALL = 1, DMX_JOINT_HINGE = 2, DMX_JOINT_SLIDER = 3, DMX_JOINT_FIXED = 4 };
typedef struct dmxJoint {
    int32_t kind, body1, body2, reserved;     /* slots; -1 = the world */
    double anchor1[3], anchor2[3];            /* in the frame of body1 / body2; world frame for a side that is -1 */
    double axis1[3], axis2[3];                /* hinge: unit axis in each side's frame; ignored for a ball */
} dmxJoint;
int dmxBatchSetJoints(dmxBatchID b, int64_t n, const dmxJoint *joints);   /* copied; replaces the set; n = 0 removes it */
int64_t dmxBatchJointCount(dmxBatchID b);
/* a joint from world-frame anchor / axis at the bodies' CURRENT poses (what dJointSetHingeAnchor / Axis mean); axis_w may be
 * NULL for a ball and for a fixed joint.  A slider takes an anchor (any point of its line) and a non-zero axis. */
int dmxBatchJointFromWorld(dmxBatchID b, int kind, int32_t body1, int32_t body2, const double anchor_w[3], const double axis_w[3],
                           dmxJoint *out);
/* per joint of the set |p2 - p1| (the anchors' separation) and, for hinges, |u x w| (0 for balls), from the current state,
 * computed on the device (inactive joints report 0); either array may be NULL; out_max[2] = the two maxima (may be NULL).
 * A slider: pos_err = the length of the part of p_2 - p_1 across u, axis_err = |2 e_v|; a fixed joint: |p_2 - p_1| and |2 e_v|
 * (e as defined at DMX_JOINT_SLIDER below, with the joint's q_0). */
int dmxBatchJointErrors(dmxBatchID b, double *pos_err, double *axis_err, double out_max[2]);

/* ---- a hinge's limits, motor and angle (dJointSetHingeParam: dParamLoStop / HiStop / Vel / FMax; dJointGetHingeAngle / Rate).
 * This is ODE's limit / motor row for a hinge with fudge factor 1, no bounce, and the world's ERP / CFM for the stop.
 *   angle   For a hinge with sides (body1, body2) AS GIVEN by the caller: q_i = the body's quaternion (a world side: the identity),
 *           q_rel = conj(q_1) q_2, q_0 = the joint's stored zero pose (q_rel when the zero was taken), e = q_rel conj(q_0) = (e_w, e_v),
 *           phi = 2 atan2(e_v . axis1, e_w) wrapped into (-pi, pi] (e and -e give the same phi).  The hinge angle is theta = -phi: the
 *           angle of body 1 relative to body 2 about u = R_1 axis1, ODE's sign.  The rate is theta_dot = u . (omega_1 - omega_2), the
 *           omega of a world side being 0.  A joint given as (world, body) reports the angle and rate of the sides as given: the
 *           internal exchange of sides changes the sign of nothing the caller sees or sets.
 *   row     A hinge whose limot is PRESENT -- fmax > 0, or a finite lo_stop, or a finite hi_stop -- has one more row, behind its five.
 *           In the sides as given J = [ 0, u | 0, -u ]: the row's velocity is theta_dot (after an exchange of sides both angular
 *           blocks change sign).  cfm = the world's CFM, k = ERP / h, g = fmax sign(vel) when fmax > 0, else 0 (sign(0) = 0).
 *           Limits are on when lo_stop <= hi_stop and at least one of the two is finite.  c, lo, hi -- the first line that matches:
 *               limits on, lo_stop == hi_stop (locked)     c = -k (theta - lo_stop)   lo = -inf    hi = +inf
 *               limits on, theta <= lo_stop                c = -k (theta - lo_stop)   lo = g       hi = +inf
 *               limits on, theta >= hi_stop                c = -k (theta - hi_stop)   lo = -inf    hi = g
 *               otherwise, fmax > 0                        c = vel                    lo = -fmax   hi = +fmax
 *               otherwise (inside its range, no motor)     c = 0                      lo = 0       hi = 0
 *           theta is the angle at the tick's start.  The shifted bound g at a stop is ODE's "motor torque applied by hand while the
 *           limit row is in use", written as one box row: the multiplier is the limit's force plus the motor's +-fmax, so the
 *           limit's own part stays >= 0.  The last line keeps a present limot at exactly one row whatever the state: the row count
 *           depends on the parameters alone.  A hinge whose limot is not present has no such row, and a tick with no present limot
 *           anywhere stages and launches exactly what it does without limots.
 * Without limots a hinge's q_0 is the identity: dmxBatchHingeAngles then reports the angle relative to the two frames coinciding. */
typedef struct dmxHingeLimot { double lo_stop, hi_stop, vel, fmax; double qrel0[4]; } dmxHingeLimot;
/* one entry per joint of the current set, whatever its kind (entries of ball joints are ignored; a slider's or a fixed joint's
 * gives its zero pose, a slider's also its stops and motor); n must equal dmxBatchJointCount or be 0 (removes them);
 * copied; may be replaced every tick (a controller setting vel / fmax).  dmxBatchSetJoints drops the limots.  DMX_EINVAL: another n,
 * a non-finite vel or fmax, a NaN stop. */
int dmxBatchSetHingeLimots(dmxBatchID b, int64_t n, const dmxHingeLimot *limots);
/* lo_stop = -inf, hi_stop = +inf, vel = fmax = 0, qrel0 = conj(q_1) q_2 at the bodies' CURRENT poses: "this pose is angle zero" */
int dmxBatchHingeLimotInit(dmxBatchID b, const dmxJoint *joint, dmxHingeLimot *out);
/* theta and theta_dot per joint of the set, from the current state, computed on the device in the batch's precision (balls and
 * inactive joints report 0); either array may be NULL */
int dmxBatchHingeAngles(dmxBatchID b, double *angle, double *rate);

/* ---- slider and fixed joints (dJointCreateSlider / dJointCreateFixed): DMX_JOINT_SLIDER, DMX_JOINT_FIXED in dmxBatchSetJoints.
 * Everything follows the conventions above: canonical sides (body1 = -1 with a live body2 exchanges the sides, anchors and axes
 * included), the activity rules, k = ERP / h, cfm = the world's, a_i = R_i anchor_i, p_i = x_i + a_i; a world side has p = anchor,
 * a = 0 and no Jacobian block.
 *   zero pose    q_0 is the qrel0 of the joint's entry in dmxBatchSetHingeLimots, which takes one entry per joint of the set whatever
 *                its kind (only a ball's entry is ignored); the identity when no limots are set, as for a hinge.
 *                dmxBatchHingeLimotInit serves any kind.  In canonical sides q_0c = q_0, or conj(q_0) after an exchange of sides.
 *   angular lock (three rows; slider and fixed)  e = conj(q_1) q_2 conj(q_0c), negated when e_w < 0; Phi = R_1 (2 e_v); for
 *                d = e_x, e_y, e_z:  J = [ 0, d | 0, -d ],  c = k Phi . d;  unbounded.  (To first order the hinge unit's c = k (u x w) . r.)
 *   slider's linear unit (two rows)  u = R_1 axis1, (p, q) = dPlaneSpace(u); for r = p, q:
 *                J = [ r, (p_2 - x_1) x r | -r, -(a_2 x r) ],  c = k (p_2 - p_1) . r;  unbounded.  The ball's row with body 1's arm taken
 *                to body 2's anchor point: the exact derivative of (p_2 - p_1) . r when r turns with body 1.
 *   position     in the sides AS GIVEN, as a hinge's angle:  s = u . (p_1 - p_2), u = R_1 axis1 of the given side 1 (a world side 1: its
 *                axis as given);  s_dot = [ u, (p_2 - x_1) x u | -u, -(a_2 x u) ] . (v_1, w_1, v_2, w_2), the exact derivative of s.
 *                When the given side 1 is the world the row in canonical form is [ -u, -(a x u) | 0 ], a = the body's arm.
 *   slider limot one row behind the slider's five, PRESENT by the hinge's rule (fmax > 0 or a finite stop); its Jacobian is the one
 *                s_dot is written with; c, lo, hi from the hinge's five-line table with s for theta: stops in metres, vel in m/s,
 *                fmax in N.  The inside-range line keeps the row (c = lo = hi = 0): the row count depends on parameters alone.
 *   row order    slider: lock (3), linear (2), limot (1 if present).  fixed: ball unit (3, the anchors as given), lock (3).
 * A set without sliders and fixed joints stages and launches exactly what it did before these kinds existed. */
/* s and s_dot per joint of the set, from the current state, computed on the device in the batch's precision (other kinds and
 * inactive joints report 0); either array may be NULL */
int dmxBatchSliderPositions(dmxBatchID b, double *pos, double *rate);

/* ---- angular motors (dJointCreateAMotor): DMX_JOINT_AMOTOR in dmxBatchSetJoints, usually beside a ball joint on the same two bodies.
 * An AMotor is a joint of the set like every other -- island building, row order, the activity rules, auto-disable, damping, feedback --
 * but its dmxJoint anchors and axes and its entry in dmxBatchSetHingeLimots are ignored: its own data is its dmxAMotor, one entry per
 * joint of the set in a table that runs beside it (dmxBatchSetAMotors), read for this kind only.  R_i = side i's rotation, the identity
 * for a world side; everything is in the sides AS GIVEN.
 *   user mode   num_axes = 1..3.  a_i = axis[i] turned by the rotation of the side rel[i] names (0: the world, as given; 1: side 1;
 *               2: side 2; a world side's frame is the world).  theta_i = angle[i], as the caller supplies it.
 *   Euler mode  num_axes = 3.  a_0 = R_1 axis[0], a_2 = R_2 axis[2], a_1 = (a_2 x a_0) / |a_2 x a_0| (the zero vector when that length
 *               is 0: nothing becomes NaN; keeping theta_1 away from +-pi/2 is the caller's duty, by stops, as in ODE).
 *               r_1 = R_1 ref1, r_2 = R_2 ref2, and
 *                   theta_0 = -atan2(a_2 . (a_0 x r_1), a_2 . r_1)
 *                   theta_1 = -atan2(a_2 . a_0, a_2 . (a_0 x a_1))
 *                   theta_2 = -atan2(r_2 . a_1, r_2 . (a_1 x a_2))           [ODE-recall: amotorComputeEulerAngles]
 *               With Z the zero pose (where ref1 = R_1^T a_2, ref2 = R_2^T a_0 were taken) and a_1 = a_2 x a_0 there: side 1 standing
 *               at Rot(a_2, theta_2) Rot(a_1, theta_1) Rot(a_0, theta_0) relative to where it stood against side 2 has these angles;
 *               each grows when side 1 turns about +a_i against side 2, the hinge angle's sign.
 *   rows        axis i < num_axes has one row when its limot is PRESENT by the hinge's rule: fmax[i] > 0 or a finite stop.  Rows come
 *               in axis order, each a unit of one row.  In the sides as given J = [ 0, a_i | 0, -a_i ] (after an exchange of sides
 *               both angular blocks change sign); c, lo, hi from the hinge's five-line table above with theta_i, k = ERP / h, cfm = the
 *               world's.  The axes and angles are those at the tick's start.
 *   rate        the row's velocity a_i . (omega_1 - omega_2): exactly theta_1's derivative for the middle Euler axis, for axes 0 and
 *               2 theta_i's only near theta_1 = 0 [ODE-recall: ODE builds the same rows].  dmxBatchAMotorAngles reports exactly this
 *               quantity as the rate -- the velocity the row acts on, not d theta_i / dt.
 * An AMotor none of whose limots is present makes no row; it still links its two bodies into one island.  A tick whose set holds no
 * AMotor with a present limot stages, launches and loads exactly what it did before this kind existed.
 * Out of scope: dJointCreateLMotor; dParamFudgeFactor, dParamBounce, dParamCFM, dParamStopERP, dParamStopCFM (fudge 1, no bounce, the
 * world's ERP / CFM, as for the hinge); an Euler-mode angle with a world side on both ends (such a joint is inactive anyway). */
enum { DMX_JOINT_AMOTOR = 5 };
enum { DMX_AMOTOR_USER = 0, DMX_AMOTOR_EULER = 1 };          /* dAMotorUser, dAMotorEuler */
typedef struct dmxAMotor {
    int32_t mode, num_axes;        /* user: 1..3; Euler: 3 */
    int32_t rel[3], pad;           /* user mode: the frame axis[i] is given in: 0 the world, 1 side 1, 2 side 2 (sides AS GIVEN; a world side's frame is the world) */
    double axis[3][3];             /* user: unit axes.  Euler: axis[0] in the frame of side 1, axis[2] in the frame of side 2, axis[1] ignored */
    double ref1[3], ref2[3];       /* Euler: reference vectors in the frames of side 1 / side 2 */
    double angle[3];               /* user mode: the angle the caller supplies per axis (dJointSetAMotorAngle); Euler: ignored */
    double lo_stop[3], hi_stop[3], vel[3], fmax[3];
} dmxAMotor;
/* one entry per joint of the current set, whatever its kind (only an AMotor's is read and checked); n must equal dmxBatchJointCount
 * or be 0 (removes them: every AMotor of the set then makes no row); copied; may be replaced every tick; dmxBatchSetJoints drops it.
 * DMX_EINVAL, one line on stderr, nothing changed: another n; for an AMotor's entry a mode or num_axes out of range, Euler with
 * num_axes != 3, a rel outside 0..2, a non-finite axis, reference, angle, vel or fmax, a NaN stop. */
int dmxBatchSetAMotors(dmxBatchID b, int64_t n, const dmxAMotor *motors);
/* an entry from world-frame axes at the bodies' CURRENT poses (what dJointSetAMotorAxis means): axes are normalised; user mode stores
 * axis[i] in the frame rel[i] names; Euler mode (rel ignored) stores axis[0] in side 1's frame, axis[2] in side 2's, and the
 * reference vectors ref1 = R_1^T a_2, ref2 = R_2^T a_0: "this pose is angles zero".  Stops -+inf, vel = fmax = angle = 0.
 * DMX_EINVAL: a bad mode, num_axes, rel or slot, a zero or non-finite axis, Euler axes 0 and 2 not perpendicular (|a_0 . a_2| > 1e-9). */
int dmxBatchAMotorFromWorld(dmxBatchID b, int32_t body1, int32_t body2, int mode, int num_axes, const int32_t rel[3],
                            const double axes_w[3][3], dmxAMotor *out);
/* three angles and three rates per joint of the set, from the current state, computed on the device in the batch's precision by the
 * kernel that prepares a tick's AMotor rows; other kinds, unused axes and inactive joints report 0; either array may be NULL.  The
 * rate is a_i . (omega_1 - omega_2), see "rate" above.  Without dmxBatchSetAMotors everything reports 0. */
int dmxBatchAMotorAngles(dmxBatchID b, double *angles3, double *rates3);

/* ---- feedback: the force and torque every joint and contact joint applied in the last tick (dJointSetFeedback).
 * A constraint with rows r = 0..m-1 in canonical sides has, per row, the Jacobian J_r = [ Jl1, Ja1 | Jl2, Ja2 ] at the tick's start,
 * unscaled, as the definitions above give it, and the multiplier lambda_r as the solve left it, after clamping -- a force: both
 * steppers solve A lambda = c/h - J (v/h + M^-1 f).  Its feedback is
 *     f1 = sum lambda_r Jl1_r,  t1 = sum lambda_r Ja1_r,  f2 = sum lambda_r Jl2_r,  t2 = sum lambda_r Ja2_r:
 * the force and the torque about each body's centre that the constraint applied to body 1 and body 2 during the tick.
 *   sides      as the caller gave them: an internal exchange of sides swaps the pairs back (as the angle and position getters do).
 *   world      a world side reports zeros.   kinematic: a kinematic side reports its J^T lambda like any other (its block of J
 *              exists although its inverse mass is zero).
 *   joints     a joint's feedback is the sum over all its units (a slider: lock + linear + limot).  At a stop the limot row's
 *              lambda includes the motor's shifted bound g: it is reported as part of the joint, as the row is defined.  Force or
 *              torque added to the bodies' accumulators by hand is no part of it.
 *   contacts   the normal row and, when mu > 0, the two friction rows.
 *   zeros      inactive joints, and contact joints the stepper dropped (no live dynamic body, or twice the same body).
 * Off by default; off, every tick stages, launches and stores exactly what it does without this section.  On, every
 * dmxBatchStepJoints tick leaves its feedback on the device (one more small launch on the general path, none in the single-launch
 * tick, which writes it to host-mapped memory); the bodies' state is bit-identical with it on and off.  The getters return
 * DMX_EINVAL with one line on stderr while feedback is off, before the first dmxBatchStepJoints tick made with it on, after any
 * other tick or write of body state (dmxBatchStep and its siblings produce none), after dmxBatchSetJoints (the last tick's
 * feedback belongs to the joints of the old set), and for an n that does not match: nothing stale is ever returned. */
typedef struct dmxJointFeedback { double f1[3], t1[3], f2[3], t2[3]; } dmxJointFeedback;
int dmxBatchSetFeedback(dmxBatchID b, int on);                        /* default 0 */
int dmxBatchJointFeedback(dmxBatchID b, dmxJointFeedback *out);       /* one per joint of the set */
/* one per contact joint of the last dmxBatchStepJoints tick, in the order given; n must equal that tick's n_joints */
int dmxBatchContactFeedback(dmxBatchID b, int64_t n, dmxJointFeedback *out);
/* device arrays of 12 reals per entry (f1, t1, f2, t2) in the batch's precision, valid until the next tick; either may be NULL */
int dmxBatchFeedbackDevice(dmxBatchID b, const void **joints_dev, const void **contacts_dev);

/* per-body flags: dBodyDestroy'ed slots, dBodySetKinematic (main.c:712), gravity / gyro modes.
 * Honoured by dmxBatchStepJoints, in every solver form and for bodies without rows: a slot without DMX_BODY_ALIVE is not
 * stepped and a joint that names it treats it as static; a KINEMATIC body keeps its velocities, moves with them and acts on
 * its joints with infinite mass; NOGRAVITY / NOGYRO leave out gravity / the gyroscopic torque of that body.  Ray casts skip
 * slots that are not alive.
 * Refused by the ticks that find their own contacts -- dmxBatchStep, dmxBatchStepTimed, dmxBatchStepRange, dmxBatchChunkTick,
 * dmxBatchChunkTicks, dmxBatchExactTick: their fused kernels never read the flags while the islands they build do, so while
 * any slot of [0, active count) has a byte other than DMX_BODY_ALIVE -- DMX_BODY_AUTODISABLE and DMX_BODY_DISABLED included,
 * these ticks know no auto-disable -- they return DMX_EINVAL, say so in one line on stderr
 * and leave the state untouched (ghost slots do not count).  Nothing is silently ignored.
 * dmxBatchFindPairs does not read the flags: a dead slot still takes part in the pair search unless its class is
 * DMX_GEOM_NONE (dmxBatchUploadGeomType), which is how the ODE face retires a destroyed body. */
enum { DMX_BODY_ALIVE = 1, DMX_BODY_KINEMATIC = 2, DMX_BODY_NOGRAVITY = 4, DMX_BODY_NOGYRO = 8,
       DMX_BODY_AUTODISABLE = 16, DMX_BODY_DISABLED = 32 };
int dmxBatchUploadBodyFlags(dmxBatchID b, const uint8_t *flags, int64_t first, int64_t count);

/* ---- auto-disable: resting bodies sleep, islands wake on contact (dmxBatchStepJoints only; off by default, as in ODE)
 * A slot is ASLEEP when its byte has DMX_BODY_ALIVE and DMX_BODY_DISABLED; DMX_BODY_AUTODISABLE lets a body fall asleep by itself.
 * Parameters of the batch: linear and angular speed thresholds (m/s, rad/s, >= 0), idle_steps (>= 0) and idle_time (seconds,
 * >= 0); anything else is DMX_EINVAL.  Defaults are ODE's [ODE-recall]: 0.01, 0.01, 10, 0.  Per slot the batch keeps steps_left
 * (int32) and time_left (a double in both precisions: a run of subtractions of h must not end on another tick in float32).  A
 * slot's counters are put back to (idle_steps, idle_time) when the batch is created, when dmxBatchSetAutoDisable is called (every
 * slot), and when dmxBatchUploadBodyFlags takes its DISABLED bit from set to clear or its AUTODISABLE bit from clear to set; an
 * upload that leaves both bits as they were leaves the counters alone.
 * Start of a dmxBatchStepJoints tick: islands are formed as always (the active articulation joints and the tick's contact joints
 * between two live slots).  An island is awake if it holds a live slot without DISABLED (a kinematic body counts like any
 * other).  In an awake island every member's DISABLED bit is cleared -- the counters are not touched [ODE-recall
 * dxProcessIslands] -- and the island is stepped as always.  An island without an awake member is left out: its bodies' state,
 * force and torque accumulators and counters keep their bits, no gravity is applied, its joints make no rows, their feedback is
 * zeros (as for dropped joints) and its contact joints do not count in dmxBatchLastContactCount.  A lone asleep body is such an
 * island.
 * End of the tick, for every slot the tick stepped that has ALIVE | AUTODISABLE and not KINEMATIC, on the post-step velocities in
 * the batch's precision:
 *     idle = (lvel.lvel <= lin_threshold^2) && (avel.avel <= ang_threshold^2)
 *     if idle:  steps_left = max(steps_left - 1, 0);  time_left = max(time_left - h, 0)
 *     else:     steps_left = idle_steps;              time_left = idle_time
 *     if steps_left == 0 && time_left == 0:  set DISABLED;  lvel = avel = 0
 * ODE evaluates the rule at the start of the next step; the two differ only if the host edits velocities between ticks.  ODE's
 * averaged samples and per-body thresholds are not offered.  Kinematic bodies never fall asleep.  Nothing but the island rule
 * and a flag upload wakes a body: uploading a pose or a force does not [ODE-recall: dBodySetPosition, dBodyAddForce].
 * Ray casts go on seeing asleep bodies; the single-launch tick's limit of 512 live bodies counts them too.
 * dmxBatchDownloadBodyFlags returns the flag bytes as they stand after every tick enqueued so far (it waits for the last tick
 * that stepped an AUTODISABLE body; so does the next tick's start, which needs the bits to build its islands).
 * dmxBatchIdleCounters: one entry per slot; either pointer may be NULL.
 * dmxBatchAutoDisableStats: [0] slots asleep now, [1] islands left out of the last tick, [2] bodies put to sleep by the rule
 * since creation, [3] bodies woken by the island rule since creation. */
int dmxBatchSetAutoDisable(dmxBatchID b, double lin_threshold, double ang_threshold, int idle_steps, double idle_time);
int dmxBatchGetAutoDisable(dmxBatchID b, double *lin_threshold, double *ang_threshold, int *idle_steps, double *idle_time);
int dmxBatchDownloadBodyFlags(dmxBatchID b, uint8_t *flags_out, int64_t first, int64_t count);
int dmxBatchIdleCounters(dmxBatchID b, int32_t *steps_left, double *time_left);
int dmxBatchAutoDisableStats(dmxBatchID b, int64_t out[4]);

/* ---- damping, maximum angular speed, contact correction (dmxBatchStepJoints only; all four are no-ops at their defaults, ODE's)
 * The rules are this library's definitions, written from ODE as recalled [ODE-recall dWorldSetDamping, dBodySetMaxAngularSpeed,
 * dWorldSetContactSurfaceLayer, dWorldSetContactMaxCorrectingVel]; the deliberate differences are named.
 * Per-slot table, one dmxBodyDamping per slot: lin_scale, ang_scale in [0, 1]; lin_threshold, ang_threshold >= 0 (m/s, rad/s);
 * max_angular_speed > 0 or +inf.  Anything else is DMX_EINVAL with nothing changed.  Defaults [ODE-recall]: 0, 0, 0.01, 0.01, +inf.
 * The table lives on the device in the batch's precision and is allocated by the first call that sets a non-default value; a
 * batch that never made one stages, launches and loads exactly what it does without this section.
 * Damping: at the start of a tick, after the islands are formed and the auto-disable wake rule has run, for every slot the tick
 * steps that is ALIVE and not KINEMATIC, on the pre-tick velocities, in the batch's precision:
 *     if lin_scale != 0 and lvel.lvel > lin_threshold^2:  lvel *= (1 - lin_scale)
 *     if ang_scale != 0 and avel.avel > ang_threshold^2:  avel *= (1 - ang_scale)
 * threshold^2 and 1 - scale are formed in the batch's precision (as the auto-disable thresholds are squared); the comparison is
 * strict.  Gravity, the gyroscopic torque, the rows' right-hand sides and the bounce rule all see the damped velocities.
 * Differences from ODE: ODE damps kinematic bodies too -- this library does not, a kinematic body keeps its velocities (above);
 * and the slots of islands left asleep are not damped: they keep their bits, like everything else of theirs.
 * Maximum angular speed: in the integrator, after the velocity update and before the pose update, for a non-kinematic slot:
 *     if avel.avel > max^2:  avel *= max / sqrt(avel.avel)
 * The quaternion advances with the capped avel.  With max = +inf the test is never true.
 * Contact surface layer and maximum correcting velocity: two scalars of the batch, surface_layer >= 0 (metres) and
 * max_correcting_vel > 0 or +inf (m/s), defaults 0 and +inf.  They act on the normal row of every contact joint of the tick:
 *     depth = max(depth - surface_layer, 0)
 *     c = (erp / h) * depth
 *     if c > max_correcting_vel:  c = max_correcting_vel
 *     then the bounce rule as always  (c = max(c, -bounce * outgoing))
 * The clamp sits between the push-out and the bounce: a bounce may exceed it, as in ODE.  Articulation rows and friction rows are
 * untouched.  At the defaults the arithmetic is depth - 0 and a comparison with +inf: bit-identical to a library without them.
 * Refused by the ticks that find their own contacts -- dmxBatchStep, dmxBatchStepTimed, dmxBatchStepRange, dmxBatchChunkTick,
 * dmxBatchChunkTicks, dmxBatchExactTick -- whose fused kernels know none of this: while the table holds a non-default entry in
 * [0, active count), or a contact scalar is not at its default, they return DMX_EINVAL, say so in one line on stderr and leave
 * the state untouched.  Nothing is silently ignored.
 * dmxBatchSetDamping / dmxBatchSetMaxAngularSpeed: every slot's four damping values / maximum speed; the other fields stand.
 * dmxBatchDownloadBodyDamping returns the defaults while no table has been made. */
typedef struct dmxBodyDamping { double lin_scale, ang_scale, lin_threshold, ang_threshold, max_angular_speed; } dmxBodyDamping;
int dmxBatchSetDamping(dmxBatchID b, double lin_scale, double ang_scale, double lin_threshold, double ang_threshold);
int dmxBatchSetMaxAngularSpeed(dmxBatchID b, double max_speed);
int dmxBatchUploadBodyDamping(dmxBatchID b, const dmxBodyDamping *damping, int64_t first, int64_t count);
int dmxBatchDownloadBodyDamping(dmxBatchID b, dmxBodyDamping *out, int64_t first, int64_t count);
int dmxBatchSetContactCorrection(dmxBatchID b, double surface_layer, double max_correcting_vel);
int dmxBatchGetContactCorrection(dmxBatchID b, double *surface_layer, double *max_correcting_vel);

/* ---- diagnostics of the last step */
int dmxBatchLastContactCount(dmxBatchID b, int64_t *n);       /* contact joints created in the last tick */
int dmxBatchLastResidual(dmxBatchID b, double *r);            /* sum |delta lambda| of the last SOR sweep */

/* ---- pose read-back for the 60 Hz snapshot (main.c:221-240): GetTransformMat (main.c:602-622) on
 * device; out_dev/out_host receive count x 16 reals, column-major 4x4 per body */
int dmxBatchPackTransforms(dmxBatchID b, void *out_dev, int64_t first, int64_t count);
int dmxBatchDownloadTransforms(dmxBatchID b, void *out_host, int64_t first, int64_t count);

/* ---- boundary-body exchange for island sharding across GPUs: gather pos+quat+lvel+avel
 * (13 reals) of the listed bodies into a contiguous device buffer (count x 13, AoS) and back */
int dmxBatchGatherBodies(dmxBatchID b, const int32_t *idx_dev, int64_t count, void *out_dev);
int dmxBatchScatterBodies(dmxBatchID b, const int32_t *idx_dev, int64_t count, const void *in_dev);
/* scatter on a caller-chosen hipStream_t (the exchange's side stream): ghost slots are never touched by the step
 * kernels, so they can be refreshed while the batch's own stream integrates the next tick */
int dmxBatchScatterBodiesOnStream(dmxBatchID b, const int32_t *idx_dev, int64_t count, const void *in_dev, void *hip_stream);

const char *dmxVersion(void);

#ifdef __cplusplus
}
#endif
#endif
