// ode_compat.cpp -- the ODE C API subset of include/ode/ode.h on top of the device batch.
//
// What runs where (the split the reference's call pattern forces):
//   host   : object bookkeeping, dSpaceCollide's pair loop and the user's near callback, dCollide (the
//            callback needs its contacts synchronously, /root/reference/src/main.c:678), grouping the
//            tick's contact joints into islands;
//   device : everything dWorldStep / dWorldQuickStep computes -- contact rows, SOR sweeps, velocity
//            update, integration (dmxBatchStepJoints -> solve_islands) -- and the pose snapshot.
// Host mirrors of body state are refreshed lazily: the first getter (or dSpaceCollide) after a step does
// one bulk device->host copy; setters mark the world dirty and the next step uploads.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "../../include/ode/ode.h"
#include "../../include/dmx_batch.h"
#include "dmx_collide.hpp"
#include "dmx_ray.hpp"
#include "dmx_math.hpp"
#include "dmx_island_rows.hpp"      // hinge_angle: the function the device builds the limit / motor row with
#include "dmx_amotor.hpp"           // amotor_axes: the function the device prepares an angular motor's axes and angles with

using dmx::M3;
using dmx::Q4;
using dmx::V3;

namespace {

#ifdef dSINGLE
constexpr int kPrecision = DMX_F32;
constexpr dReal kDefaultCFM = 1e-5f;
#else
constexpr int kPrecision = DMX_F64;
constexpr dReal kDefaultCFM = 1e-10;
#endif

[[noreturn]] void fatal(const char *what, int rc)
{
    fprintf(stderr, "libode_mi355: %s failed (code %d); the step has no CPU fallback\n", what, rc);
    abort();
}
#define DMX_MUST(call) do { int rc_ = (call); if (rc_ != DMX_OK) fatal(#call, rc_); } while (0)

M3<dReal> to_m3(const dReal *R) { return { { { R[0], R[1], R[2] }, { R[4], R[5], R[6] }, { R[8], R[9], R[10] } } }; }
void from_m3(const M3<dReal> &M, dReal *R)
{
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) R[4 * i + j] = M.m[i][j]; R[4 * i + 3] = 0; }
}
void set_identity(dReal *R) { memset(R, 0, 12 * sizeof(dReal)); R[0] = R[5] = R[10] = 1; }

}  // namespace

struct dxGeom;
struct dxJoint;

struct dxBody {
    dxWorld *world = nullptr;
    int slot = -1;
    dVector3 pos = { 0, 0, 0, 0 };
    dMatrix3 R;
    dQuaternion q = { 1, 0, 0, 0 };
    dVector3 lvel = { 0, 0, 0, 0 }, avel = { 0, 0, 0, 0 };
    dVector3 facc = { 0, 0, 0, 0 }, tacc = { 0, 0, 0, 0 };
    dMass mass;
    int flags = DMX_BODY_ALIVE;
    dmxBodyDamping damp = { 0.0, 0.0, 0.01, 0.01, __builtin_huge_val() };      // dBodySetDamping & co.: the world's at creation
    std::vector<dxGeom *> geoms;
};

struct dxGeom {
    int cls = dBoxClass;
    int id = 0;                       // creation order: fixes the pair order of dSpaceCollide
    dxBody *body = nullptr;
    dxSpace *space = nullptr;
    dReal side[3] = { 0, 0, 0 };      // box sides / sphere radius in side[0]
    dReal plane[4] = { 0, 0, 1, 0 };
    dVector3 pos = { 0, 0, 0, 0 };    // pose of a body-less (static) geom, main.c:748-749
    dMatrix3 R;
    unsigned long cat = ~0ul, col = ~0ul;
};

struct dxSpace {
    std::vector<dxGeom *> geoms;
};

struct dxJoint {
    dxWorld *world = nullptr;
    dxJointGroup *group = nullptr;
    dContact contact;
    dxBody *b1 = nullptr, *b2 = nullptr;
    int type = dJointTypeContact;
    // a ball, a hinge, a slider or a fixed joint: anchors and axes in the frames of the two bodies (world frame for a side without a body)
    double anchor1[3] = { 0, 0, 0 }, anchor2[3] = { 0, 0, 0 }, axis1[3] = { 1, 0, 0 }, axis2[3] = { 1, 0, 0 };
    // a hinge's or a slider's limit and motor (dJointSetHingeParam / dJointSetSliderParam) and the zero pose -- a slider's and a fixed
    // joint's too --, conj(q_1) q_2 of the sides AS ATTACHED when the anchor or
    // the axis was last set (include/dmx_batch.h, dmxHingeLimot).  rev: attached as (0, body) -- b1 / b2 above are exchanged, and
    // the angle, the rate, the stops and the motor are those of the sides as attached [ODE-recall dJOINT_REVERSE: dJointGetHingeAngle
    // and dJointAddHingeTorque change sign]
    bool rev = false;
    double lo_stop = -__builtin_huge_val(), hi_stop = __builtin_huge_val(), vel = 0, fmax = 0;
    double qrel0[4] = { 1, 0, 0, 0 };
    dJointFeedback *fb = nullptr;      // dJointSetFeedback: the caller's struct, filled by every step while it is set
    // an angular motor (dJointCreateAMotor): its dmxAMotor in the sides AS ATTACHED -- rel 1 / 2 name the bodies the caller attached
    // first / second, also after dJointAttach(j, 0, body) -- with num_axes as the caller set it (0 .. 3: the batch is handed a blank
    // entry for 0); am_set: bit i = axis i has been given
    dmxAMotor am = {};
    int am_set = 0;
};

struct dxJointGroup {
    std::vector<dxJoint *> joints;
};

struct dxWorld {
    dmxBatchID batch = nullptr;
    int cap = 0;
    std::vector<dxBody *> slots;       // slot -> body (nullptr = free)
    std::vector<dxJoint *> joints;     // contact joints of the current tick, creation order
    std::vector<dxJoint *> arts;       // ball, hinge, slider and fixed joints, creation order: they persist (dmxBatchSetJoints)
    bool art_dirty = false;            // ... and changed since the batch last saw them
    bool limot_dirty = false;          // a hinge's limit / motor parameter or zero pose changed since the batch last saw them
    bool limots_sent = false;          // the batch holds limots (dmxBatchSetHingeLimots)
    bool amotor_dirty = false;         // an angular motor's mode, axes, angles or parameters changed since the batch last saw them
    std::vector<dmxAMotor> am;
    int n_feedback = 0;                // joints of the world with a feedback struct set (dJointSetFeedback)
    bool feedback_sent = false;        // the batch's feedback is switched on (dmxBatchSetFeedback): only while n_feedback > 0
    std::vector<dmxJointFeedback> fbuf;
    std::vector<dmxJoint> aj;
    std::vector<dmxHingeLimot> al;
    dReal g[3] = { 0, 0, 0 };
    dReal erp = (dReal)0.2, cfm = kDefaultCFM, sor_w = (dReal)1.3;
    int iters = 20;
    bool dev_newer = false;            // device holds newer body state than the host mirrors
    bool host_dirty = true;            // host mirrors hold changes the device has not seen
    uint32_t order_seed = 0; bool order_seeded = false;     // DMX_ROW_ORDER=ode:<seed>
    bool geom_dirty = true;            // the bodies' geoms (class, extents) changed since the device last saw them
    std::vector<double> dev_statics;   // the static boxes the device holds (18 doubles each), for the device pair search
    std::vector<dReal> buf;
    std::vector<dmxContactJoint> cj;
    std::vector<dmxContactSurface> cs;         // the rest of the tick's surfaces; handed over only when some contact sets one of its bits
    // auto-disable (dWorldSetAutoDisable*).  The four values are the world's and hold for all its bodies (stock ODE copies them
    // into a body at creation); the flag is what dBodyCreate copies.  ad_dirty: the batch has not been told the values yet.
    // n_ad: bodies whose flags carry DMX_BODY_AUTODISABLE or DMX_BODY_DISABLED -- only while there is one does to_host() ask the
    // batch for the flag bytes; a world that never touches the feature makes no call it did not make before.
    bool ad_flag = false, ad_dirty = false;
    double ad_lin = 0.01, ad_ang = 0.01, ad_time = 0.0;
    int ad_steps = 10, n_ad = 0;
    std::vector<uint8_t> flbuf;
    // damping, maximum angular speed, contact correction (dWorldSetDamping & co.; include/dmx_batch.h, "damping").  damp: what
    // dBodyCreate copies into a new body.  damp_used: some body has ever held a non-default entry -- only then does a step send
    // the table (damp_dirty: it changed since); cc_dirty: the batch has not been told the two contact scalars yet.  A world that
    // never touches any of this makes no call it did not make before; a world that outgrows its batch sends both again.
    dmxBodyDamping damp = { 0.0, 0.0, 0.01, 0.01, __builtin_huge_val() };
    double surface_layer = 0.0, max_corr_vel = __builtin_huge_val();
    bool damp_used = false, damp_dirty = false, cc_dirty = false;
    std::vector<dmxBodyDamping> dbuf;
    void push_damping()
    {
        if (damp_dirty) {
            const dmxBodyDamping def = { 0.0, 0.0, 0.01, 0.01, __builtin_huge_val() };
            dbuf.assign((size_t)cap, def);
            for (int s = 0; s < cap; s++) if (slots[(size_t)s]) dbuf[(size_t)s] = slots[(size_t)s]->damp;
            DMX_MUST(dmxBatchUploadBodyDamping(batch, dbuf.data(), 0, cap));
            damp_dirty = false;
        }
        if (cc_dirty) {
            DMX_MUST(dmxBatchSetContactCorrection(batch, surface_layer, max_corr_vel));
            cc_dirty = false;
        }
    }
    void set_flags(dxBody *b, int flags)
    {
        const int bits = DMX_BODY_AUTODISABLE | DMX_BODY_DISABLED;
        n_ad += (int)((flags & bits) != 0) - (int)((b->flags & bits) != 0);
        b->flags = flags;
    }

    void create_batch(int capacity)
    {
        DMX_MUST(dmxBatchCreate(&batch, capacity, kPrecision, 0));
        if (const char *e = getenv("DMX_ROW_ORDER")) {          // "ode" or "ode:<seed>": stock ODE's row order and shuffle for dWorldQuickStep
            if (strncmp(e, "ode", 3) == 0) {
                if (!order_seeded) { order_seed = e[3] == ':' ? (uint32_t)strtoul(e + 4, nullptr, 10) : 0u; order_seeded = true; }
                DMX_MUST(dmxBatchSetRowOrder(batch, DMX_ORDER_ODE, order_seed));
            }
        }
        cap = capacity;
        slots.resize((size_t)cap, nullptr);
        host_dirty = true;
        pushed_valid = false;          // a new batch has been told nothing yet
        art_dirty = !arts.empty();
        feedback_sent = false;         // (a new batch's feedback is off: world_step switches it on again if a struct is set)
        ad_dirty = ad_lin != 0.01 || ad_ang != 0.01 || ad_steps != 10 || ad_time != 0.0;      // (a new batch holds the defaults)
        damp_dirty = damp_used;
        cc_dirty = surface_layer != 0.0 || max_corr_vel != __builtin_huge_val();
        // One read-back the general way into the buffer to_host() uses, now.  The runtime registers a pageable destination the
        // first time a device-to-host copy lands in it (8 ms, measured); a world whose ticks run on the single-launch path reads
        // its poses from the batch's host mirror and would meet that at the first tick that falls back -- a whole 120 Hz frame.
        buf.assign((size_t)cap * 13, 0);
        DMX_MUST(dmxBatchDownload(batch, DMX_STATE, buf.data(), 0, cap));
    }
    // what the batch was last told (push_params): a tick pushes the world's parameters only when one has changed since
    dReal pushed[7] = { 0, 0, 0, 0, 0, 0, 0 }; int pushed_iters = 0, pushed_stepper = -1; bool pushed_valid = false;
    void push_params(int stepper)
    {
        const dReal now[7] = { g[0], g[1], g[2], erp, cfm, sor_w, (dReal)0 };
        if (pushed_valid && memcmp(now, pushed, sizeof(now)) == 0 && pushed_iters == iters && pushed_stepper == stepper) return;
        DMX_MUST(dmxBatchSetGravity(batch, g[0], g[1], g[2]));
        DMX_MUST(dmxBatchSetERP(batch, erp));
        DMX_MUST(dmxBatchSetCFM(batch, cfm));
        DMX_MUST(dmxBatchSetQuickStep(batch, iters, sor_w));
        DMX_MUST(dmxBatchSetStepper(batch, stepper));
        memcpy(pushed, now, sizeof(now)); pushed_iters = iters; pushed_stepper = stepper; pushed_valid = true;
    }
    void to_host()
    {
        if (!dev_newer) return;
        // one transfer for the whole read-back (13 reals per slot: pos3 quat4 lvel3 avel3), up to the highest live slot
        int hi = 0;
        for (int s = 0; s < cap; s++) if (slots[(size_t)s]) hi = s + 1;
        buf.resize((size_t)hi * 13);
        if (hi > 0) DMX_MUST(dmxBatchDownload(batch, DMX_STATE, buf.data(), 0, hi));
        for (int s = 0; s < hi; s++) {
            dxBody *b = slots[(size_t)s];
            if (!b) continue;
            const dReal *r = &buf[(size_t)s * 13];
            for (int k = 0; k < 3; k++) { b->pos[k] = r[k]; b->lvel[k] = r[7 + k]; b->avel[k] = r[10 + k]; }
            for (int k = 0; k < 4; k++) b->q[k] = r[3 + k];
        }
        if (n_ad > 0 && hi > 0) {
            // the DISABLED bits the ticks set or cleared come back too: to_device() uploads every slot's flags from dxBody::flags,
            // and a stale byte there would wake a sleeper or put a woken body back to sleep
            flbuf.resize((size_t)hi);
            DMX_MUST(dmxBatchDownloadBodyFlags(batch, flbuf.data(), 0, hi));
            for (int s = 0; s < hi; s++)
                if (dxBody *b = slots[(size_t)s]) set_flags(b, (b->flags & ~DMX_BODY_DISABLED) | (flbuf[(size_t)s] & DMX_BODY_DISABLED));
        }
        for (dxBody *b : slots) {
            if (!b) continue;
            const Q4<dReal> q = { b->q[0], b->q[1], b->q[2], b->q[3] };
            from_m3(dmx::quat_to_R(q), b->R);          // dxStepBody: R = R(q)
            b->facc[0] = b->facc[1] = b->facc[2] = 0;  // the step cleared the accumulators
            b->tacc[0] = b->tacc[1] = b->tacc[2] = 0;
        }
        dev_newer = false;
    }
    void to_device()
    {
        if (!host_dirty) return;
        to_host();
        auto up = [&](int field, int k, auto get) {
            buf.assign((size_t)cap * k, 0);
            for (int s = 0; s < cap; s++) {
                const dxBody *b = slots[(size_t)s];
                for (int j = 0; j < k; j++) buf[(size_t)s * k + j] = b ? get(b, j) : (dReal)(field == DMX_STATE ? (j == 3) : (field == DMX_MASS || field == DMX_INERTIA));   // empty slot: unit quaternion, unit mass
            }
            DMX_MUST(dmxBatchUpload(batch, field, buf.data(), 0, cap));
        };
        // pos3 quat4 lvel3 avel3 in one transfer; the quaternion is already normalised and is stored as is
        up(DMX_STATE, 13, [](const dxBody *b, int j) { return j < 3 ? b->pos[j] : j < 7 ? b->q[j - 3] : j < 10 ? b->lvel[j - 7] : b->avel[j - 10]; });
        up(DMX_MASS, 1, [](const dxBody *b, int) { return b->mass.mass; });
        up(DMX_INERTIA, 3, [](const dxBody *b, int j) { return b->mass.I[5 * j]; });
        up(DMX_FORCE, 3, [](const dxBody *b, int j) { return b->facc[j]; });
        up(DMX_TORQUE, 3, [](const dxBody *b, int j) { return b->tacc[j]; });
        std::vector<uint8_t> fl((size_t)cap, 0);
        for (int s = 0; s < cap; s++) if (slots[(size_t)s]) fl[(size_t)s] = (uint8_t)slots[(size_t)s]->flags;
        DMX_MUST(dmxBatchUploadBodyFlags(batch, fl.data(), 0, cap));
        host_dirty = false;
    }
    // extents and classes of the bodies' geoms, for the device pair search (dSpaceCollide); false when some body's
    // geometry is not one box / sphere geom (the host search handles those worlds)
    bool geometry_to_device();
    void grow()
    {
        to_host();
        std::vector<dxBody *> keep = slots;
        DMX_MUST(dmxBatchDestroy(batch));
        batch = nullptr;
        create_batch(cap * 2);
        std::copy(keep.begin(), keep.end(), slots.begin());
        geom_dirty = true;
        dev_statics.clear();
    }
};

namespace {

int g_next_geom_id = 0;

const dReal *geom_pos(const dxGeom *g) { return g->body ? g->body->pos : g->pos; }
const dReal *geom_R(const dxGeom *g) { return g->body ? g->body->R : g->R; }
void touch(dxBody *b) { b->world->to_host(); b->world->host_dirty = true; }
void sync_geom(const dxGeom *g) { if (g->body) g->body->world->to_host(); }

}  // namespace

bool dxWorld::geometry_to_device()
{
    if (!geom_dirty) return true;
    std::vector<dReal> sides((size_t)cap * 3, 0);
    std::vector<uint8_t> gt((size_t)cap, DMX_GEOM_NONE);
    for (int s = 0; s < cap; s++) {
        const dxBody *b = slots[(size_t)s];
        if (!b || b->geoms.empty()) continue;                  // a body without geoms collides with nothing
        if (b->geoms.size() != 1) return false;
        const dxGeom *g = b->geoms[0];
        if (g->cls == dBoxClass) { gt[(size_t)s] = DMX_GEOM_BOX; for (int k = 0; k < 3; k++) sides[(size_t)s * 3 + k] = g->side[k]; }
        else if (g->cls == dSphereClass) { gt[(size_t)s] = DMX_GEOM_SPHERE; sides[(size_t)s * 3] = g->side[0]; }
        else return false;
    }
    DMX_MUST(dmxBatchUpload(batch, DMX_SIDES, sides.data(), 0, cap));
    DMX_MUST(dmxBatchUploadGeomType(batch, gt.data(), 0, cap));
    geom_dirty = false;
    return true;
}

// ================================================================================ lifecycle
extern "C" void dInitODE(void) { (void)dInitODE2(0); }
extern "C" int dInitODE2(unsigned int)
{
    if (dmxDeviceCount() < 1) {
        fprintf(stderr, "libode_mi355: dInitODE: no MI355X / HIP device visible; this library has no CPU path\n");
        return 0;
    }
    return 1;
}
extern "C" void dCloseODE(void) {}

// ================================================================================ world
extern "C" dWorldID dWorldCreate(void)
{
    dxWorld *w = new dxWorld();
    w->create_batch(512);              // MAX_BODIES, inc/body.h:6; doubles on demand
    return w;
}
extern "C" void dWorldDestroy(dWorldID w)
{
    if (!w) return;
    for (dxBody *b : w->slots) {
        if (!b) continue;
        for (dxGeom *g : b->geoms) g->body = nullptr;
        delete b;
    }
    for (dxJoint *j : w->joints) j->world = nullptr;
    // ball and hinge joints outside a group go with the world; those in a group are the group's to delete [ODE-recall dWorldDestroy]
    for (dxJoint *j : w->arts) { if (j->group) j->world = nullptr; else delete j; }
    if (w->batch) dmxBatchDestroy(w->batch);
    delete w;
}
extern "C" void dWorldSetGravity(dWorldID w, dReal x, dReal y, dReal z) { w->g[0] = x; w->g[1] = y; w->g[2] = z; }
extern "C" void dWorldGetGravity(dWorldID w, dVector3 g) { g[0] = w->g[0]; g[1] = w->g[1]; g[2] = w->g[2]; }
extern "C" void dWorldSetERP(dWorldID w, dReal erp) { w->erp = erp; }
extern "C" dReal dWorldGetERP(dWorldID w) { return w->erp; }
extern "C" void dWorldSetCFM(dWorldID w, dReal cfm) { w->cfm = cfm; }
extern "C" dReal dWorldGetCFM(dWorldID w) { return w->cfm; }
extern "C" void dWorldSetQuickStepNumIterations(dWorldID w, int n) { w->iters = n; }
extern "C" int dWorldGetQuickStepNumIterations(dWorldID w) { return w->iters; }
extern "C" void dWorldSetQuickStepW(dWorldID w, dReal v) { w->sor_w = v; }
extern "C" dReal dWorldGetQuickStepW(dWorldID w) { return w->sor_w; }
// auto-disable: the flag is what dBodyCreate copies into a new body; the four values are the world's and hold for ALL its bodies
// from the next step on -- stock ODE copies them into a body at creation and lets dBodySetAutoDisable* change them per body
// [ODE-recall]; setting one resets every body's idle counters (dmxBatchSetAutoDisable)
extern "C" void dWorldSetAutoDisableFlag(dWorldID w, int do_auto_disable) { w->ad_flag = do_auto_disable != 0; }
extern "C" int dWorldGetAutoDisableFlag(dWorldID w) { return w->ad_flag ? 1 : 0; }
extern "C" void dWorldSetAutoDisableLinearThreshold(dWorldID w, dReal v) { if (v >= 0) { w->ad_lin = v; w->ad_dirty = true; } }
extern "C" dReal dWorldGetAutoDisableLinearThreshold(dWorldID w) { return (dReal)w->ad_lin; }
extern "C" void dWorldSetAutoDisableAngularThreshold(dWorldID w, dReal v) { if (v >= 0) { w->ad_ang = v; w->ad_dirty = true; } }
extern "C" dReal dWorldGetAutoDisableAngularThreshold(dWorldID w) { return (dReal)w->ad_ang; }
extern "C" void dWorldSetAutoDisableSteps(dWorldID w, int steps) { if (steps >= 0) { w->ad_steps = steps; w->ad_dirty = true; } }
extern "C" int dWorldGetAutoDisableSteps(dWorldID w) { return w->ad_steps; }
extern "C" void dWorldSetAutoDisableTime(dWorldID w, dReal t) { if (t >= 0) { w->ad_time = t; w->ad_dirty = true; } }
extern "C" dReal dWorldGetAutoDisableTime(dWorldID w) { return (dReal)w->ad_time; }
extern "C" void dWorldSetAutoDisableAverageSamplesCount(dWorldID, unsigned int n)
{
    if (n != 1) fprintf(stderr, "libode_mi355: dWorldSetAutoDisableAverageSamplesCount: %u is not supported (the idle test looks at one sample, the step's own); ignored\n", n);
}
extern "C" int dWorldGetAutoDisableAverageSamplesCount(dWorldID) { return 1; }

// damping, maximum angular speed, contact correction (include/dmx_batch.h, "damping").  One place says what a value may be.
namespace {
bool damp_value_ok(const char *who, bool ok, double v)
{
    if (!ok) fprintf(stderr, "libode_mi355: %s: %g is out of range; ignored\n", who, v);
    return ok;
}
bool damp_entry_default(const dmxBodyDamping &d)
{
    // (in dReal, the width the values were given in: dBodySetLinearDampingThreshold(b, 0.01f) of the single-precision build sets the
    //  default, though (double)0.01f is not the double 0.01)
    return d.lin_scale == 0 && d.ang_scale == 0 && (dReal)d.lin_threshold == (dReal)0.01 && (dReal)d.ang_threshold == (dReal)0.01 &&
           d.max_angular_speed == __builtin_huge_val();
}
void body_damping_changed(dxBody *b)
{
    dxWorld *w = b->world;
    if (!w->damp_used && damp_entry_default(b->damp)) return;
    w->damp_used = true; w->damp_dirty = true;
}
}  // namespace
extern "C" void dWorldSetLinearDamping(dWorldID w, dReal v) { if (damp_value_ok("dWorldSetLinearDamping", v >= 0 && v <= 1, v)) w->damp.lin_scale = v; }
extern "C" dReal dWorldGetLinearDamping(dWorldID w) { return (dReal)w->damp.lin_scale; }
extern "C" void dWorldSetAngularDamping(dWorldID w, dReal v) { if (damp_value_ok("dWorldSetAngularDamping", v >= 0 && v <= 1, v)) w->damp.ang_scale = v; }
extern "C" dReal dWorldGetAngularDamping(dWorldID w) { return (dReal)w->damp.ang_scale; }
extern "C" void dWorldSetDamping(dWorldID w, dReal lin, dReal ang) { dWorldSetLinearDamping(w, lin); dWorldSetAngularDamping(w, ang); }
extern "C" void dWorldSetLinearDampingThreshold(dWorldID w, dReal v) { if (damp_value_ok("dWorldSetLinearDampingThreshold", v >= 0, v)) w->damp.lin_threshold = v; }
extern "C" dReal dWorldGetLinearDampingThreshold(dWorldID w) { return (dReal)w->damp.lin_threshold; }
extern "C" void dWorldSetAngularDampingThreshold(dWorldID w, dReal v) { if (damp_value_ok("dWorldSetAngularDampingThreshold", v >= 0, v)) w->damp.ang_threshold = v; }
extern "C" dReal dWorldGetAngularDampingThreshold(dWorldID w) { return (dReal)w->damp.ang_threshold; }
extern "C" void dWorldSetMaxAngularSpeed(dWorldID w, dReal v) { if (damp_value_ok("dWorldSetMaxAngularSpeed", v > 0, v)) w->damp.max_angular_speed = v; }
extern "C" dReal dWorldGetMaxAngularSpeed(dWorldID w) { return (dReal)w->damp.max_angular_speed; }
extern "C" void dWorldSetContactSurfaceLayer(dWorldID w, dReal v)
{ if (damp_value_ok("dWorldSetContactSurfaceLayer", v >= 0 && v < dInfinity, v)) { w->surface_layer = v; w->cc_dirty = true; } }
extern "C" dReal dWorldGetContactSurfaceLayer(dWorldID w) { return (dReal)w->surface_layer; }
extern "C" void dWorldSetContactMaxCorrectingVel(dWorldID w, dReal v)
{ if (damp_value_ok("dWorldSetContactMaxCorrectingVel", v > 0, v)) { w->max_corr_vel = v; w->cc_dirty = true; } }
extern "C" dReal dWorldGetContactMaxCorrectingVel(dWorldID w) { return (dReal)w->max_corr_vel; }

static int world_step(dWorldID w, dReal h, int stepper)
{
    if (!w || !(h > 0)) return 0;
    w->to_device();
    w->push_params(stepper);
    if (w->ad_dirty) {                 // (resets every slot's idle counters: include/dmx_batch.h)
        DMX_MUST(dmxBatchSetAutoDisable(w->batch, w->ad_lin, w->ad_ang, w->ad_steps, w->ad_time));
        w->ad_dirty = false;
    }
    w->push_damping();
    if (w->art_dirty) {               // the articulation joints go to the batch only when they changed
        w->aj.clear();
        for (const dxJoint *j : w->arts) {
            dmxJoint a;
            memset(&a, 0, sizeof a);
            // (the batch's enum does not take ODE's numbering: kind 7 stays refused there)
            a.kind = j->type == dJointTypeHinge ? DMX_JOINT_HINGE : j->type == dJointTypeSlider ? DMX_JOINT_SLIDER :
                     j->type == dJointTypeFixed ? DMX_JOINT_FIXED : j->type == dJointTypeAMotor ? DMX_JOINT_AMOTOR : DMX_JOINT_BALL;
            a.body1 = j->b1 ? j->b1->slot : -1;
            a.body2 = j->b2 ? j->b2->slot : -1;
            for (int k = 0; k < 3; k++) { a.anchor1[k] = j->anchor1[k]; a.anchor2[k] = j->anchor2[k]; a.axis1[k] = j->axis1[k]; a.axis2[k] = j->axis2[k]; }
            if (j->rev && j->b1 && !j->b2) {
                // the sides as attached, (0, body): the batch exchanges them as dJointAttach did -- the same five rows -- and its
                // limit / motor row and angle are those of the sides as given
                a.body1 = -1; a.body2 = j->b1->slot;
                for (int k = 0; k < 3; k++) { a.anchor1[k] = j->anchor2[k]; a.anchor2[k] = j->anchor1[k]; a.axis1[k] = j->axis2[k]; a.axis2[k] = j->axis1[k]; }
            }
            w->aj.push_back(a);
        }
        DMX_MUST(dmxBatchSetJoints(w->batch, (int64_t)w->aj.size(), w->aj.data()));
        w->art_dirty = false;
        w->limots_sent = false;        // (dmxBatchSetJoints drops them)
        w->limot_dirty = true;
        w->amotor_dirty = true;        // (... and the angular motors' table)
    }
    if (w->amotor_dirty) {             // the angular motors' table, when the joints or one of its values changed; none: nothing is sent
        w->am.clear();
        bool any = false;
        for (const dxJoint *j : w->arts) {
            dmxAMotor m = j->am;
            if (j->type != dJointTypeAMotor || m.num_axes < 1) {
                memset(&m, 0, sizeof m);
                m.num_axes = 1;
                for (int i = 0; i < 3; i++) { m.lo_stop[i] = -__builtin_huge_val(); m.hi_stop[i] = __builtin_huge_val(); }
            }
            any = any || j->type == dJointTypeAMotor;
            w->am.push_back(m);
        }
        if (any) DMX_MUST(dmxBatchSetAMotors(w->batch, (int64_t)w->am.size(), w->am.data()));
        w->amotor_dirty = false;
    }
    if (w->limot_dirty) {              // ... and the hinges' limits and motors when the joints or a parameter changed
        w->al.clear();
        bool any = false;
        for (const dxJoint *j : w->arts) {
            dmxHingeLimot l;
            l.lo_stop = j->lo_stop; l.hi_stop = j->hi_stop; l.vel = j->vel; l.fmax = j->fmax;
            for (int k = 0; k < 4; k++) l.qrel0[k] = j->qrel0[k];
            if ((j->type == dJointTypeHinge || j->type == dJointTypeSlider) && dmx::limot_present(l.lo_stop, l.hi_stop, l.fmax)) any = true;
            if (j->type == dJointTypeSlider || j->type == dJointTypeFixed) any = true;      // (their zero pose is part of their rows)
            w->al.push_back(l);
        }
        // (a world without sliders and fixed joints none of whose hinges has a limit or a motor hands the batch nothing: its ticks
        //  are what they were without them)
        if (any) { DMX_MUST(dmxBatchSetHingeLimots(w->batch, (int64_t)w->al.size(), w->al.data())); w->limots_sent = true; }
        else if (w->limots_sent) { DMX_MUST(dmxBatchSetHingeLimots(w->batch, 0, nullptr)); w->limots_sent = false; }
        w->limot_dirty = false;
    }
    w->cj.clear();
    w->cs.clear();
    bool extended = false;      // dContactMu2 / FDir1 / Motion1 / 2 / N / Slip1 / 2 somewhere in this tick's contacts
    for (const dxJoint *j : w->joints) {
        dmxContactJoint c;
        const dContact &ct = j->contact;
        for (int k = 0; k < 3; k++) { c.pos[k] = ct.geom.pos[k]; c.normal[k] = ct.geom.normal[k]; }
        c.depth = ct.geom.depth;
        c.body1 = j->b1 ? j->b1->slot : -1;
        c.body2 = j->b2 ? j->b2->slot : -1;
        c.mode = ct.surface.mode;
        c.mu = ct.surface.mu; c.bounce = ct.surface.bounce; c.bounce_vel = ct.surface.bounce_vel;
        c.soft_erp = ct.surface.soft_erp; c.soft_cfm = ct.surface.soft_cfm;
        w->cj.push_back(c);
        dmxContactSurface sf;
        sf.mu2 = ct.surface.mu2; sf.motion1 = ct.surface.motion1; sf.motion2 = ct.surface.motion2; sf.motionN = ct.surface.motionN;
        sf.slip1 = ct.surface.slip1; sf.slip2 = ct.surface.slip2;
        for (int k = 0; k < 3; k++) sf.fdir1[k] = ct.fdir1[k];
        w->cs.push_back(sf);
        if (c.mode & DMX_CONTACT_SURFACE_EXT) extended = true;
    }
    // feedback: on in the batch only while some joint of the world has a struct set -- a world without one ticks as it always did
    const bool feedback = w->n_feedback > 0;
    if (feedback != w->feedback_sent) { DMX_MUST(dmxBatchSetFeedback(w->batch, feedback ? 1 : 0)); w->feedback_sent = feedback; }
    {
        // (a tick none of whose contacts sets one of the seven bits makes the call it always made)
        const int rc = extended ? dmxBatchStepJointsSurface(w->batch, h, (int64_t)w->cj.size(), w->cj.data(), w->cs.data())
                                : dmxBatchStepJoints(w->batch, h, (int64_t)w->cj.size(), w->cj.data());
        // ball / hinge joints under DMX_ROW_ORDER=ode with QuickStep: the batch has said so on stderr; the step fails, the process lives
        if (rc == DMX_EINVAL && !w->arts.empty()) return 0;
        // an extended surface the batch refuses (a NaN, a negative or infinite slip, an infinite motion or fdir1 in a dContact; such a
        // tick under DMX_ROW_ORDER=ode with QuickStep): likewise -- one line on stderr from the batch, the bodies where they were
        if (rc == DMX_EINVAL && extended) return 0;
        if (rc != DMX_OK) fatal(extended ? "dmxBatchStepJointsSurface" : "dmxBatchStepJoints", rc);
    }
    w->dev_newer = true;
    if (feedback) {
        // the batch reports the sides as it was given them; f1 / t1 here belong to dJointGetBody(j, 0): an articulation joint
        // attached as (0, body) was handed over as (world, body) and has the body as its body 1
        auto fill = [](const dmxJointFeedback &s, bool exchange, dJointFeedback *d) {
            const double *a = exchange ? s.f2 : s.f1, *b = exchange ? s.t2 : s.t1, *c = exchange ? s.f1 : s.f2, *e = exchange ? s.t1 : s.t2;
            for (int k = 0; k < 3; k++) { d->f1[k] = (dReal)a[k]; d->t1[k] = (dReal)b[k]; d->f2[k] = (dReal)c[k]; d->t2[k] = (dReal)e[k]; }
            d->f1[3] = d->t1[3] = d->f2[3] = d->t2[3] = 0;
        };
        bool arts = false, contacts = false;
        for (const dxJoint *j : w->arts) arts = arts || j->fb;
        for (const dxJoint *j : w->joints) contacts = contacts || j->fb;
        if (arts) {
            w->fbuf.resize(w->arts.size());
            DMX_MUST(dmxBatchJointFeedback(w->batch, w->fbuf.data()));
            for (size_t k = 0; k < w->arts.size(); k++)
                if (w->arts[k]->fb) fill(w->fbuf[k], w->arts[k]->rev && w->arts[k]->b1 && !w->arts[k]->b2, w->arts[k]->fb);
        }
        if (contacts) {
            w->fbuf.resize(w->joints.size());
            DMX_MUST(dmxBatchContactFeedback(w->batch, (int64_t)w->joints.size(), w->fbuf.data()));
            for (size_t k = 0; k < w->joints.size(); k++)
                if (w->joints[k]->fb) fill(w->fbuf[k], false, w->joints[k]->fb);
        }
    }
    return 1;
}
// dWorldQuickStep: QuickStep's SOR sweeps.  dWorldStep -- what the reference calls, main.c:213 -- the same rows with
// every island's LCP solved exactly (include/dmx_batch.h, dmxBatchSetStepper).
extern "C" int dWorldQuickStep(dWorldID w, dReal h) { return world_step(w, h, DMX_STEPPER_QUICK); }
extern "C" int dWorldStep(dWorldID w, dReal h) { return world_step(w, h, DMX_STEPPER_EXACT); }

// ================================================================================ mass
extern "C" void dMassSetZero(dMass *m) { memset(m, 0, sizeof(*m)); }
extern "C" void dMassSetParameters(dMass *m, dReal themass, dReal cgx, dReal cgy, dReal cgz, dReal I11, dReal I22,
                                   dReal I33, dReal I12, dReal I13, dReal I23)
{
    dMassSetZero(m);
    m->mass = themass;
    m->c[0] = cgx; m->c[1] = cgy; m->c[2] = cgz;
    m->I[0] = I11; m->I[5] = I22; m->I[10] = I33;
    m->I[1] = m->I[4] = I12; m->I[2] = m->I[8] = I13; m->I[6] = m->I[9] = I23;
}
extern "C" void dMassSetBoxTotal(dMass *m, dReal total, dReal lx, dReal ly, dReal lz)
{
    dMassSetZero(m);
    m->mass = total;
    m->I[0] = total / (dReal)12.0 * (ly * ly + lz * lz);
    m->I[5] = total / (dReal)12.0 * (lx * lx + lz * lz);
    m->I[10] = total / (dReal)12.0 * (lx * lx + ly * ly);
}
extern "C" void dMassSetBox(dMass *m, dReal density, dReal lx, dReal ly, dReal lz)
{ dMassSetBoxTotal(m, lx * ly * lz * density, lx, ly, lz); }
extern "C" void dMassSetSphereTotal(dMass *m, dReal total, dReal r)
{
    dMassSetZero(m);
    m->mass = total;
    const dReal II = (dReal)0.4 * total * r * r;
    m->I[0] = m->I[5] = m->I[10] = II;
}
extern "C" void dMassSetSphere(dMass *m, dReal density, dReal r)
{ dMassSetSphereTotal(m, (dReal)(4.0 / 3.0 * 3.14159265358979323846) * r * r * r * density, r); }

// ================================================================================ bodies
extern "C" dBodyID dBodyCreate(dWorldID w)
{
    if (!w) return nullptr;
    int slot = -1;
    for (int s = 0; s < w->cap; s++) if (!w->slots[(size_t)s]) { slot = s; break; }
    if (slot < 0) { slot = w->cap; w->grow(); }
    w->to_host();
    dxBody *b = new dxBody();
    b->world = w;
    b->slot = slot;
    set_identity(b->R);
    dMassSetParameters(&b->mass, 1, 0, 0, 0, 1, 1, 1, 0, 0, 0);   // ODE default; the reference never sets mass (F7)
    w->slots[(size_t)slot] = b;
    w->host_dirty = true;
    if (w->ad_flag) w->set_flags(b, b->flags | DMX_BODY_AUTODISABLE);      // dBodySetAutoDisableDefaults
    b->damp = w->damp;                                                     // dBodySetDampingDefaults
    body_damping_changed(b);
    return b;
}
extern "C" void dBodyDestroy(dBodyID b)
{
    if (!b) return;
    dxWorld *w = b->world;
    w->to_host();
    for (dxGeom *g : b->geoms) g->body = nullptr;
    for (dxJoint *j : w->joints) { if (j->b1 == b) j->b1 = nullptr; if (j->b2 == b) j->b2 = nullptr; }
    // its articulation joints are detached on both sides, ODE's limbo: inactive until attached again
    for (dxJoint *j : w->arts) if (j->b1 == b || j->b2 == b) { j->b1 = j->b2 = nullptr; w->art_dirty = true; }
    w->set_flags(b, DMX_BODY_ALIVE);      // (out of the count of bodies with an auto-disable bit)
    if (w->damp_used) w->damp_dirty = true;      // (its slot goes back to the defaults)
    w->slots[(size_t)b->slot] = nullptr;
    w->host_dirty = true;
    delete b;
}
extern "C" dWorldID dBodyGetWorld(dBodyID b) { return b->world; }
extern "C" void dBodySetPosition(dBodyID b, dReal x, dReal y, dReal z) { touch(b); b->pos[0] = x; b->pos[1] = y; b->pos[2] = z; }
extern "C" void dBodySetRotation(dBodyID b, const dMatrix3 R)
{
    touch(b);
    memcpy(b->R, R, sizeof(dMatrix3));
    b->R[3] = b->R[7] = b->R[11] = 0;
    Q4<dReal> q = dmx::R_to_quat(to_m3(b->R));
    dmx::normalize(q);
    b->q[0] = q.w; b->q[1] = q.x; b->q[2] = q.y; b->q[3] = q.z;
}
extern "C" void dBodySetQuaternion(dBodyID b, const dQuaternion qq)
{
    touch(b);
    Q4<dReal> q = { qq[0], qq[1], qq[2], qq[3] };
    dmx::normalize(q);
    b->q[0] = q.w; b->q[1] = q.x; b->q[2] = q.y; b->q[3] = q.z;
    from_m3(dmx::quat_to_R(q), b->R);
}
extern "C" void dBodySetLinearVel(dBodyID b, dReal x, dReal y, dReal z) { touch(b); b->lvel[0] = x; b->lvel[1] = y; b->lvel[2] = z; }
extern "C" void dBodySetAngularVel(dBodyID b, dReal x, dReal y, dReal z) { touch(b); b->avel[0] = x; b->avel[1] = y; b->avel[2] = z; }
extern "C" const dReal *dBodyGetPosition(dBodyID b) { b->world->to_host(); return b->pos; }
extern "C" const dReal *dBodyGetRotation(dBodyID b) { b->world->to_host(); return b->R; }
extern "C" const dReal *dBodyGetQuaternion(dBodyID b) { b->world->to_host(); return b->q; }
extern "C" const dReal *dBodyGetLinearVel(dBodyID b) { b->world->to_host(); return b->lvel; }
extern "C" const dReal *dBodyGetAngularVel(dBodyID b) { b->world->to_host(); return b->avel; }
extern "C" void dBodySetKinematic(dBodyID b) { touch(b); b->flags |= DMX_BODY_KINEMATIC; }
extern "C" void dBodySetDynamic(dBodyID b) { touch(b); b->flags &= ~DMX_BODY_KINEMATIC; }
extern "C" int dBodyIsKinematic(dBodyID b) { return (b->flags & DMX_BODY_KINEMATIC) != 0; }
extern "C" void dBodySetGyroscopicMode(dBodyID b, int on) { touch(b); if (on) b->flags &= ~DMX_BODY_NOGYRO; else b->flags |= DMX_BODY_NOGYRO; }
extern "C" int dBodyGetGyroscopicMode(dBodyID b) { return (b->flags & DMX_BODY_NOGYRO) == 0; }
// auto-disable (include/dmx_batch.h, "auto-disable").  touch() brings the DISABLED bits the ticks left back first, so the upload
// of every slot's flags that follows a change changes this body's byte only.  dBodyEnable clears DISABLED, which resets the
// body's idle counters in the batch; dBodyDisable sets it and leaves the velocities as they are [ODE-recall].
extern "C" void dBodySetAutoDisableFlag(dBodyID b, int do_auto_disable)
{
    touch(b);
    // (switching it off also enables the body [ODE-recall dBodySetAutoDisableFlag: "reset the IsDisabled state"])
    b->world->set_flags(b, do_auto_disable ? b->flags | DMX_BODY_AUTODISABLE : b->flags & ~(DMX_BODY_AUTODISABLE | DMX_BODY_DISABLED));
}
extern "C" int dBodyGetAutoDisableFlag(dBodyID b) { return (b->flags & DMX_BODY_AUTODISABLE) != 0; }
extern "C" void dBodySetAutoDisableDefaults(dBodyID b) { dBodySetAutoDisableFlag(b, b->world->ad_flag ? 1 : 0); }
extern "C" void dBodyEnable(dBodyID b) { touch(b); b->world->set_flags(b, b->flags & ~DMX_BODY_DISABLED); }
extern "C" void dBodyDisable(dBodyID b) { touch(b); b->world->set_flags(b, b->flags | DMX_BODY_DISABLED); }
extern "C" int dBodyIsEnabled(dBodyID b) { b->world->to_host(); return (b->flags & DMX_BODY_DISABLED) == 0; }
// damping and the maximum angular speed of one body: the table goes to the batch at the next step
extern "C" void dBodySetLinearDamping(dBodyID b, dReal v) { if (damp_value_ok("dBodySetLinearDamping", v >= 0 && v <= 1, v)) { b->damp.lin_scale = v; body_damping_changed(b); } }
extern "C" dReal dBodyGetLinearDamping(dBodyID b) { return (dReal)b->damp.lin_scale; }
extern "C" void dBodySetAngularDamping(dBodyID b, dReal v) { if (damp_value_ok("dBodySetAngularDamping", v >= 0 && v <= 1, v)) { b->damp.ang_scale = v; body_damping_changed(b); } }
extern "C" dReal dBodyGetAngularDamping(dBodyID b) { return (dReal)b->damp.ang_scale; }
extern "C" void dBodySetDamping(dBodyID b, dReal lin, dReal ang) { dBodySetLinearDamping(b, lin); dBodySetAngularDamping(b, ang); }
extern "C" void dBodySetLinearDampingThreshold(dBodyID b, dReal v) { if (damp_value_ok("dBodySetLinearDampingThreshold", v >= 0, v)) { b->damp.lin_threshold = v; body_damping_changed(b); } }
extern "C" dReal dBodyGetLinearDampingThreshold(dBodyID b) { return (dReal)b->damp.lin_threshold; }
extern "C" void dBodySetAngularDampingThreshold(dBodyID b, dReal v) { if (damp_value_ok("dBodySetAngularDampingThreshold", v >= 0, v)) { b->damp.ang_threshold = v; body_damping_changed(b); } }
extern "C" dReal dBodyGetAngularDampingThreshold(dBodyID b) { return (dReal)b->damp.ang_threshold; }
extern "C" void dBodySetMaxAngularSpeed(dBodyID b, dReal v) { if (damp_value_ok("dBodySetMaxAngularSpeed", v > 0, v)) { b->damp.max_angular_speed = v; body_damping_changed(b); } }
extern "C" dReal dBodyGetMaxAngularSpeed(dBodyID b) { return (dReal)b->damp.max_angular_speed; }
extern "C" void dBodySetDampingDefaults(dBodyID b) { b->damp = b->world->damp; body_damping_changed(b); }
extern "C" void dBodyAddForce(dBodyID b, dReal x, dReal y, dReal z) { touch(b); b->facc[0] += x; b->facc[1] += y; b->facc[2] += z; }
extern "C" void dBodyAddTorque(dBodyID b, dReal x, dReal y, dReal z) { touch(b); b->tacc[0] += x; b->tacc[1] += y; b->tacc[2] += z; }
extern "C" void dBodySetMass(dBodyID b, const dMass *m)
{
    touch(b);
    if (!(m->mass > 0) || !(m->I[0] > 0) || !(m->I[5] > 0) || !(m->I[10] > 0)) {
        fprintf(stderr, "libode_mi355: dBodySetMass: mass and principal inertia must be positive; ignored\n");
        return;
    }
    if (m->I[1] != 0 || m->I[2] != 0 || m->I[6] != 0 || m->c[0] != 0 || m->c[1] != 0 || m->c[2] != 0)
        fprintf(stderr, "libode_mi355: dBodySetMass: off-diagonal inertia / offset centre of mass are not "
                        "supported on the device path; using the diagonal about the body origin\n");
    b->mass = *m;
}
extern "C" void dBodyGetMass(dBodyID b, dMass *m) { *m = b->mass; }

// ================================================================================ spaces / geoms
extern "C" dSpaceID dSimpleSpaceCreate(dSpaceID) { return new dxSpace(); }
extern "C" dSpaceID dHashSpaceCreate(dSpaceID) { return new dxSpace(); }
extern "C" void dSpaceDestroy(dSpaceID s)
{
    if (!s) return;
    for (dxGeom *g : s->geoms) g->space = nullptr;
    delete s;
}
extern "C" int dSpaceGetNumGeoms(dSpaceID s) { return (int)s->geoms.size(); }

static dxGeom *new_geom(dSpaceID space, int cls)
{
    dxGeom *g = new dxGeom();
    g->cls = cls;
    g->id = g_next_geom_id++;
    set_identity(g->R);
    g->space = space;
    if (space) space->geoms.push_back(g);
    return g;
}
extern "C" dGeomID dCreateBox(dSpaceID space, dReal lx, dReal ly, dReal lz)
{
    dxGeom *g = new_geom(space, dBoxClass);
    g->side[0] = lx; g->side[1] = ly; g->side[2] = lz;
    return g;
}
extern "C" dGeomID dCreateSphere(dSpaceID space, dReal radius)
{
    dxGeom *g = new_geom(space, dSphereClass);
    g->side[0] = radius;
    return g;
}
extern "C" dGeomID dCreatePlane(dSpaceID space, dReal a, dReal b, dReal c, dReal d)
{
    dxGeom *g = new_geom(space, dPlaneClass);
    dReal l = a * a + b * b + c * c;
    if (l > 0) { l = (dReal)1 / dmx::tsqrt<dReal>(l); a *= l; b *= l; c *= l; d *= l; }
    else { a = 1; b = 0; c = 0; d = 0; }
    g->plane[0] = a; g->plane[1] = b; g->plane[2] = c; g->plane[3] = d;
    return g;
}
// ---- rays (include/ode/ode.h): position = the start, side[0] = the length, plane[0..2] = the unit direction
extern "C" dGeomID dCreateRay(dSpaceID space, dReal length)
{
    if (space) {
        fprintf(stderr, "libode_mi355: dCreateRay: rays do not take part in dSpaceCollide; only space == 0 is supported\n");
        return nullptr;
    }
    dxGeom *g = new_geom(nullptr, dRayClass);
    g->side[0] = length;
    g->plane[0] = 0; g->plane[1] = 0; g->plane[2] = 1; g->plane[3] = 0;       // ODE's ray points along +z until set
    return g;
}
extern "C" void dGeomRaySet(dGeomID g, dReal px, dReal py, dReal pz, dReal dx, dReal dy, dReal dz)
{
    if (!g || g->cls != dRayClass) return;
    g->pos[0] = px; g->pos[1] = py; g->pos[2] = pz;
    const dReal l = dmx::tsqrt<dReal>(dx * dx + dy * dy + dz * dz);
    if (l > 0) { dx /= l; dy /= l; dz /= l; }
    g->plane[0] = dx; g->plane[1] = dy; g->plane[2] = dz;
}
extern "C" void dGeomRayGet(dGeomID g, dVector3 start, dVector3 dir)
{
    if (!g || g->cls != dRayClass) return;
    for (int i = 0; i < 3; i++) { start[i] = g->pos[i]; dir[i] = g->plane[i]; }
    start[3] = 0; dir[3] = 0;
}
extern "C" void dGeomRaySetLength(dGeomID g, dReal length) { if (g && g->cls == dRayClass) g->side[0] = length; }
extern "C" dReal dGeomRayGetLength(dGeomID g) { return g && g->cls == dRayClass ? g->side[0] : (dReal)0; }

extern "C" void dGeomDestroy(dGeomID g)
{
    if (!g) return;
    if (g->body) { auto &v = g->body->geoms; v.erase(std::remove(v.begin(), v.end(), g), v.end()); g->body->world->geom_dirty = true; }
    if (g->space) { auto &v = g->space->geoms; v.erase(std::remove(v.begin(), v.end(), g), v.end()); }
    delete g;
}
extern "C" void dGeomSetBody(dGeomID g, dBodyID b)
{
    if (g->body == b) return;
    if (g->body) { auto &v = g->body->geoms; v.erase(std::remove(v.begin(), v.end(), g), v.end()); g->body->world->geom_dirty = true; }
    g->body = b;
    if (b) { b->geoms.push_back(g); b->world->geom_dirty = true; }
}
extern "C" dBodyID dGeomGetBody(dGeomID g) { return g->body; }
extern "C" void dGeomSetPosition(dGeomID g, dReal x, dReal y, dReal z)
{
    if (g->body) { dBodySetPosition(g->body, x, y, z); return; }
    g->pos[0] = x; g->pos[1] = y; g->pos[2] = z;
}
extern "C" void dGeomSetRotation(dGeomID g, const dMatrix3 R)
{
    if (g->body) { dBodySetRotation(g->body, R); return; }
    memcpy(g->R, R, sizeof(dMatrix3));
    g->R[3] = g->R[7] = g->R[11] = 0;
}
extern "C" const dReal *dGeomGetPosition(dGeomID g) { sync_geom(g); return geom_pos(g); }
extern "C" const dReal *dGeomGetRotation(dGeomID g) { sync_geom(g); return geom_R(g); }
extern "C" void dGeomSetCategoryBits(dGeomID g, unsigned long bits) { g->cat = bits; }
extern "C" void dGeomSetCollideBits(dGeomID g, unsigned long bits) { g->col = bits; }
extern "C" unsigned long dGeomGetCategoryBits(dGeomID g) { return g->cat; }
extern "C" unsigned long dGeomGetCollideBits(dGeomID g) { return g->col; }
extern "C" int dGeomGetClass(dGeomID g) { return g->cls; }
extern "C" void dGeomBoxGetLengths(dGeomID g, dVector3 r) { r[0] = g->side[0]; r[1] = g->side[1]; r[2] = g->side[2]; }
extern "C" dReal dGeomSphereGetRadius(dGeomID g) { return g->side[0]; }
extern "C" void dGeomPlaneGetParams(dGeomID g, dVector4 r) { for (int i = 0; i < 4; i++) r[i] = g->plane[i]; }

// ---- dCollide ------------------------------------------------------------------------------------
namespace {

struct Hit { V3<dReal> pos, normal; dReal depth; };

// contacts of the ordered class pair (a,b); false when no collider exists for that order
bool collide_ordered(const dxGeom *a, const dxGeom *b, int maxc, Hit *out, int *n)
{
    const dReal *pa = geom_pos(a), *pb = geom_pos(b);
    const V3<dReal> xa = { pa[0], pa[1], pa[2] }, xb = { pb[0], pb[1], pb[2] };
    *n = 0;
    if (a->cls == dBoxClass && b->cls == dPlaneClass) {
        V3<dReal> cp[4]; dReal cd[4];
        const V3<dReal> pn = { b->plane[0], b->plane[1], b->plane[2] };
        *n = dmx::box_plane(xa, to_m3(geom_R(a)), a->side, pn, b->plane[3], maxc, cp, cd);
        for (int i = 0; i < *n; i++) out[i] = { cp[i], pn, cd[i] };
        return true;
    }
    if (a->cls == dSphereClass && b->cls == dPlaneClass) {
        V3<dReal> cp[4]; dReal cd[4];
        const V3<dReal> pn = { b->plane[0], b->plane[1], b->plane[2] };
        *n = dmx::sphere_plane(xa, a->side[0], pn, b->plane[3], cp, cd);
        for (int i = 0; i < *n; i++) out[i] = { cp[i], pn, cd[i] };
        return true;
    }
    if (a->cls == dSphereClass && b->cls == dSphereClass) {
        dmx::ContactPoint<dReal> c;
        *n = dmx::sphere_sphere(xa, a->side[0], xb, b->side[0], &c);
        if (*n) out[0] = { c.pos, c.normal, c.depth };
        return true;
    }
    if (a->cls == dSphereClass && b->cls == dBoxClass) {
        dmx::ContactPoint<dReal> c;
        *n = dmx::sphere_box(xa, a->side[0], xb, to_m3(geom_R(b)), b->side, &c);
        if (*n) out[0] = { c.pos, c.normal, c.depth };
        return true;
    }
    if (a->cls == dBoxClass && b->cls == dBoxClass) {
        dmx::ContactPoint<dReal> c[8];
        *n = dmx::box_box(xa, to_m3(geom_R(a)), a->side, xb, to_m3(geom_R(b)), b->side, maxc, c);
        for (int i = 0; i < *n; i++) out[i] = { c[i].pos, c[i].normal, c[i].depth };
        return true;
    }
    return false;
}

}  // namespace

namespace {
// dCollide with a ray on either side: one contact at most, g1 = the ray
int collide_ray(dxGeom *ray, dxGeom *g, dContactGeom *c)
{
    if (g->cls == dRayClass) return 0;
    sync_geom(g);
    dmx::Ray<dReal> r;
    if (!dmx::ray_make<dReal>(ray->pos[0], ray->pos[1], ray->pos[2], ray->plane[0], ray->plane[1], ray->plane[2], ray->side[0], r)) return 0;
    dmx::RayHit<dReal> h;
    bool hit = false;
    if (g->cls == dPlaneClass) hit = dmx::ray_plane<dReal>(r, V3<dReal>{ g->plane[0], g->plane[1], g->plane[2] }, g->plane[3], h);
    else {
        const dReal *p = geom_pos(g);
        const V3<dReal> x = { p[0], p[1], p[2] };
        if (g->cls == dSphereClass) hit = dmx::ray_sphere<dReal>(r, x, g->side[0], h);
        else if (g->cls == dBoxClass) hit = dmx::ray_box<dReal>(r, x, to_m3(geom_R(g)), V3<dReal>{ g->side[0], g->side[1], g->side[2] }, h);
    }
    if (!hit) return 0;
    c->pos[0] = r.o.x + h.t * r.d.x; c->pos[1] = r.o.y + h.t * r.d.y; c->pos[2] = r.o.z + h.t * r.d.z; c->pos[3] = 0;
    c->normal[0] = h.n.x; c->normal[1] = h.n.y; c->normal[2] = h.n.z; c->normal[3] = 0;
    c->depth = h.t;
    c->g1 = ray; c->g2 = g;
    c->side1 = -1; c->side2 = -1;
    return 1;
}
}  // namespace

extern "C" int dCollide(dGeomID o1, dGeomID o2, int flags, dContactGeom *contact, int skip)
{
    if (!o1 || !o2 || !contact || o1 == o2) return 0;
    if (o1->cls == dRayClass) return collide_ray(o1, o2, contact);
    if (o2->cls == dRayClass) return collide_ray(o2, o1, contact);
    if (o1->body && o1->body == o2->body) return 0;
    int maxc = flags & 0xffff;
    if (maxc < 1) maxc = 1;
    sync_geom(o1); sync_geom(o2);
    Hit hits[8];
    int n = 0;
    bool flip = false;
    if (!collide_ordered(o1, o2, maxc > 8 ? 8 : maxc, hits, &n)) {
        if (!collide_ordered(o2, o1, maxc > 8 ? 8 : maxc, hits, &n)) return 0;   // e.g. plane-plane
        flip = true;
    }
    if (n > maxc) n = maxc;
    for (int i = 0; i < n; i++) {
        dContactGeom *c = (dContactGeom *)((char *)contact + (size_t)i * (size_t)skip);   // byte stride, main.c:678
        c->pos[0] = hits[i].pos.x; c->pos[1] = hits[i].pos.y; c->pos[2] = hits[i].pos.z; c->pos[3] = 0;
        const dReal sg = flip ? (dReal)-1 : (dReal)1;
        c->normal[0] = flip ? -hits[i].normal.x : hits[i].normal.x;
        c->normal[1] = flip ? -hits[i].normal.y : hits[i].normal.y;
        c->normal[2] = flip ? -hits[i].normal.z : hits[i].normal.z;
        c->normal[3] = 0; (void)sg;
        c->depth = hits[i].depth;
        c->g1 = o1; c->g2 = o2;
        c->side1 = -1; c->side2 = -1;
    }
    return n;
}

// ---- dSpaceCollide -----------------------------------------------------------------------------------
namespace {

struct GeomBox { dReal lo[3], hi[3]; };
GeomBox aabb_of(const dxGeom *g)
{
    const dReal *p = geom_pos(g), *R = geom_R(g);
    GeomBox b;
    for (int i = 0; i < 3; i++) {
        const dReal r = g->cls == dSphereClass
                            ? g->side[0]
                            : (dReal)0.5 * (dmx::tabs(R[4 * i] * g->side[0]) + dmx::tabs(R[4 * i + 1] * g->side[1]) +
                                            dmx::tabs(R[4 * i + 2] * g->side[2]));
        b.lo[i] = p[i] - r; b.hi[i] = p[i] + r;
    }
    return b;
}
bool boxes_overlap(const GeomBox &a, const GeomBox &b)
{
    return !(b.lo[0] > a.hi[0] || a.lo[0] > b.hi[0] || b.lo[1] > a.hi[1] || a.lo[1] > b.hi[1] || b.lo[2] > a.hi[2] || a.lo[2] > b.hi[2]);
}
bool pair_passes(const dxGeom *a, const dxGeom *b)
{
    if (a->body && a->body == b->body) return false;
    return ((a->cat & b->col) || (b->cat & a->col)) != 0;
}

// worlds of at least this many bodies take their body pairs from the device (DMX_COMPAT_DEVICE_PAIRS: 1 = always, 0 = never;
// a number >= 2 = that many bodies).  Below it the host sweep is quicker than a device round trip.
int device_pairs_threshold()
{
    static const int v = [] {
        const char *e = getenv("DMX_COMPAT_DEVICE_PAIRS");
        if (!e) return 2048;
        const int x = atoi(e);
        return x == 0 ? 0x7fffffff : x;
    }();
    return v;
}

// The pair search of dSpaceCollide on the device: body-body AABB pairs and the bodies near static boxes come from
// dmxBatchFindPairs (hashed-grid search, dmx_exact.hip); planes, the static boxes' own pairs and the category / collide
// filter are a few host loops over that short list.  false = this space is not of the shape the device search covers
// (bodies of several worlds, bodies with several geoms, static geoms other than boxes and planes): the host search runs.
bool device_pairs(dxSpace *space, std::vector<std::pair<dxGeom *, dxGeom *>> &pairs)
{
    dxWorld *w = nullptr;
    std::vector<dxGeom *> planes, statics;
    int nbodies = 0;
    for (dxGeom *g : space->geoms) {
        if (g->cls == dPlaneClass) { planes.push_back(g); continue; }
        if (!g->body) { if (g->cls != dBoxClass) return false; statics.push_back(g); continue; }
        if (w && g->body->world != w) return false;
        w = g->body->world;
        nbodies++;
    }
    if (!w || nbodies < device_pairs_threshold() || (int)statics.size() > DMX_MAX_STATIC_BOXES) return false;
    for (const dxBody *b : w->slots) if (b) for (const dxGeom *g : b->geoms) if (g->space != space) return false;
    w->to_device();
    if (!w->geometry_to_device()) return false;
    std::vector<double> st;
    for (const dxGeom *g : statics) {
        for (int k = 0; k < 3; k++) st.push_back(g->side[k]);
        for (int k = 0; k < 3; k++) st.push_back(g->pos[k]);
        for (int k = 0; k < 12; k++) st.push_back(g->R[k]);
    }
    if (st != w->dev_statics) {
        std::vector<double> sides, pos, rot;
        for (size_t s = 0; s < statics.size(); s++) {
            sides.insert(sides.end(), st.begin() + 18 * s, st.begin() + 18 * s + 3);
            pos.insert(pos.end(), st.begin() + 18 * s + 3, st.begin() + 18 * s + 6);
            rot.insert(rot.end(), st.begin() + 18 * s + 6, st.begin() + 18 * s + 18);
        }
        DMX_MUST(dmxBatchSetStaticBoxes(w->batch, (int32_t)statics.size(), sides.data(), pos.data(), rot.data()));
        w->dev_statics = st;
    }
    const int32_t *bp = nullptr, *inv = nullptr;
    int64_t nbp = 0, ninv = 0;
    DMX_MUST(dmxBatchFindPairs(w->batch, &bp, &nbp, &inv, &ninv));
    w->to_host();                                 // dCollide reads poses from the host mirrors: one bulk copy per tick
    auto push = [&](dxGeom *a, dxGeom *b) { if (a->id < b->id) pairs.emplace_back(a, b); else pairs.emplace_back(b, a); };
    for (int64_t k = 0; k < nbp; k++) {
        dxGeom *a = w->slots[(size_t)bp[2 * k]]->geoms[0], *b = w->slots[(size_t)bp[2 * k + 1]]->geoms[0];
        if (pair_passes(a, b)) push(a, b);
    }
    std::vector<GeomBox> sbox;
    for (const dxGeom *g : statics) sbox.push_back(aabb_of(g));
    for (int64_t k = 0; k < ninv; k++) {
        dxGeom *g = w->slots[(size_t)inv[k]]->geoms[0];
        const GeomBox gb = aabb_of(g);
        for (size_t s = 0; s < statics.size(); s++)
            if (boxes_overlap(gb, sbox[s]) && pair_passes(g, statics[s])) push(g, statics[s]);
    }
    for (size_t s = 0; s < statics.size(); s++)               // static-static pairs reach the callback too (SURVEY a-5)
        for (size_t t = s + 1; t < statics.size(); t++)
            if (boxes_overlap(sbox[s], sbox[t]) && pair_passes(statics[s], statics[t])) push(statics[s], statics[t]);
    for (dxGeom *pl : planes)
        for (dxGeom *g : space->geoms)
            if (g->cls != dPlaneClass && pair_passes(pl, g)) push(pl, g);
    return true;
}

}  // namespace

extern "C" void dSpaceCollide(dSpaceID space, void *data, dNearCallback *callback)
{
    if (!space || !callback) return;
    {
        std::vector<std::pair<dxGeom *, dxGeom *>> dpairs;
        if (device_pairs(space, dpairs)) {
            std::sort(dpairs.begin(), dpairs.end(), [](const auto &a, const auto &b) {
                return a.first->id < b.first->id || (a.first->id == b.first->id && a.second->id < b.second->id);
            });
            for (auto &pr : dpairs) callback(data, pr.first, pr.second);          // NearCallback, main.c:674
            return;
        }
    }
    struct Box { dReal lo[3], hi[3]; dxGeom *g; };
    std::vector<Box> bb;
    std::vector<dxGeom *> planes;
    std::vector<std::pair<dxGeom *, dxGeom *>> pairs;
    for (dxGeom *g : space->geoms) sync_geom(g);
    for (dxGeom *g : space->geoms) {
        if (g->cls == dPlaneClass) { planes.push_back(g); continue; }
        const dReal *p = geom_pos(g), *R = geom_R(g);
        Box b; b.g = g;
        for (int i = 0; i < 3; i++) {
            const dReal r = g->cls == dSphereClass
                                ? g->side[0]
                                : (dReal)0.5 * (dmx::tabs(R[4 * i] * g->side[0]) + dmx::tabs(R[4 * i + 1] * g->side[1]) +
                                                dmx::tabs(R[4 * i + 2] * g->side[2]));
            b.lo[i] = p[i] - r; b.hi[i] = p[i] + r;
        }
        bb.push_back(b);
    }
    auto passes = [](const dxGeom *a, const dxGeom *b) {
        if (a->body && a->body == b->body) return false;
        return ((a->cat & b->col) || (b->cat & a->col)) != 0;
    };
    auto push = [&](dxGeom *a, dxGeom *b) { if (a->id < b->id) pairs.emplace_back(a, b); else pairs.emplace_back(b, a); };
    for (dxGeom *pl : planes)
        for (const Box &b : bb) if (passes(pl, b.g)) push(pl, b.g);
    std::sort(bb.begin(), bb.end(), [](const Box &a, const Box &b) { return a.lo[0] < b.lo[0] || (a.lo[0] == b.lo[0] && a.g->id < b.g->id); });
    for (size_t i = 0; i < bb.size(); i++)
        for (size_t j = i + 1; j < bb.size() && bb[j].lo[0] <= bb[i].hi[0]; j++) {
            if (bb[j].lo[1] > bb[i].hi[1] || bb[i].lo[1] > bb[j].hi[1]) continue;
            if (bb[j].lo[2] > bb[i].hi[2] || bb[i].lo[2] > bb[j].hi[2]) continue;
            if (passes(bb[i].g, bb[j].g)) push(bb[i].g, bb[j].g);
        }
    // pair order is fixed by geom creation order so a tick is reproducible
    std::sort(pairs.begin(), pairs.end(), [](const auto &a, const auto &b) {
        return a.first->id < b.first->id || (a.first->id == b.first->id && a.second->id < b.second->id);
    });
    for (auto &pr : pairs) callback(data, pr.first, pr.second);          // NearCallback, main.c:674
}

// ================================================================================ contact joints
extern "C" dJointGroupID dJointGroupCreate(int) { return new dxJointGroup(); }
extern "C" void dJointGroupEmpty(dJointGroupID g)
{
    if (!g) return;
    for (dxJoint *j : g->joints) {
        if (j->world) {
            auto &v = j->type == dJointTypeContact ? j->world->joints : j->world->arts;
            v.erase(std::remove(v.begin(), v.end(), j), v.end());
            if (j->type != dJointTypeContact) j->world->art_dirty = true;
            if (j->fb) j->world->n_feedback--;
        }
        delete j;
    }
    g->joints.clear();
}
extern "C" void dJointGroupDestroy(dJointGroupID g) { dJointGroupEmpty(g); delete g; }
extern "C" dJointID dJointCreateContact(dWorldID w, dJointGroupID g, const dContact *c)
{
    if (!w || !c) return nullptr;
    dxJoint *j = new dxJoint();
    j->world = w;
    j->group = g;
    j->contact = *c;                   // the caller's dContact lives on its stack (main.c:676)
    w->joints.push_back(j);
    if (g) g->joints.push_back(j);
    return j;
}
extern "C" void dJointAttach(dJointID j, dBodyID b1, dBodyID b2)
{
    if (!j) return;
    j->b1 = b1; j->b2 = b2;
    if (j->type != dJointTypeContact) {
        // an articulation joint attached as (0, body): ODE exchanges the two, so that body 1 is the body [ODE-recall dJointAttach, dJOINT_REVERSE]
        j->rev = !j->b1 && j->b2;
        if (j->rev) { j->b1 = j->b2; j->b2 = nullptr; }
        if (j->world) j->world->art_dirty = true;
    }
}

// ================================================================================ ball, hinge, slider and fixed joints
namespace {

dJointID create_art(dWorldID w, dJointGroupID g, int type)
{
    if (!w) return nullptr;
    dxJoint *j = new dxJoint();
    j->world = w;
    j->group = g;
    j->type = type;
    w->arts.push_back(j);
    if (g) g->joints.push_back(j);
    w->art_dirty = true;
    return j;
}
// a world-frame point / direction into the frame of body b at its current pose, and back (b = 0: the world frame itself)
void to_body(const dxBody *b, const double in[3], bool point, double out[3])
{
    if (!b) { for (int k = 0; k < 3; k++) out[k] = in[k]; return; }
    double d[3];
    for (int k = 0; k < 3; k++) d[k] = in[k] - (point ? (double)b->pos[k] : 0.0);
    for (int k = 0; k < 3; k++) out[k] = (double)b->R[k] * d[0] + (double)b->R[4 + k] * d[1] + (double)b->R[8 + k] * d[2];      // R^T d
}
void to_world(const dxBody *b, const double in[3], bool point, dReal out[4])
{
    for (int k = 0; k < 3; k++)
        out[k] = b ? (dReal)((double)b->R[4 * k] * in[0] + (double)b->R[4 * k + 1] * in[1] + (double)b->R[4 * k + 2] * in[2] + (point ? (double)b->pos[k] : 0.0))
                   : (dReal)in[k];
}
// the two sides AS ATTACHED (rev: the first is the world) and their quaternions (a world side: the identity)
void given_sides(const dxJoint *j, const dxBody *&g1, const dxBody *&g2, dmx::Q4<double> &q1, dmx::Q4<double> &q2)
{
    g1 = j->rev ? nullptr : j->b1;
    g2 = j->rev ? j->b1 : j->b2;
    q1 = q2 = { 1.0, 0.0, 0.0, 0.0 };
    if (g1) q1 = { (double)g1->q[0], (double)g1->q[1], (double)g1->q[2], (double)g1->q[3] };
    if (g2) q2 = { (double)g2->q[0], (double)g2->q[1], (double)g2->q[2], (double)g2->q[3] };
}
// "this pose is angle zero" [ODE-recall dxJointHinge::computeInitialRelativeRotation, from dJointSetHingeAnchor / Axis]
void take_zero_pose(dJointID j)
{
    if (j->type != dJointTypeHinge && j->type != dJointTypeSlider && j->type != dJointTypeFixed) return;
    const dxBody *g1, *g2;
    dmx::Q4<double> q1, q2;
    given_sides(j, g1, g2, q1, q2);
    const dmx::Q4<double> r = dmx::qmul(dmx::qconj(q1), q2);
    j->qrel0[0] = r.w; j->qrel0[1] = r.x; j->qrel0[2] = r.y; j->qrel0[3] = r.z;
    if (j->world) j->world->limot_dirty = true;
}
void set_anchor(dJointID j, dReal x, dReal y, dReal z)
{
    if (!j || j->type == dJointTypeContact) return;
    if (j->world) j->world->to_host();
    const double p[3] = { (double)x, (double)y, (double)z };
    to_body(j->b1, p, true, j->anchor1);
    to_body(j->b2, p, true, j->anchor2);
    take_zero_pose(j);
    if (j->world) j->world->art_dirty = true;
}
void get_anchor(dJointID j, int side, dVector3 out)
{
    if (!j) return;
    if (j->world) j->world->to_host();
    to_world(side ? j->b2 : j->b1, side ? j->anchor2 : j->anchor1, true, out);
}

}  // namespace

extern "C" dJointID dJointCreateBall(dWorldID w, dJointGroupID g) { return create_art(w, g, dJointTypeBall); }
extern "C" dJointID dJointCreateHinge(dWorldID w, dJointGroupID g) { return create_art(w, g, dJointTypeHinge); }
extern "C" void dJointDestroy(dJointID j)
{
    if (!j) return;
    if (j->world) {
        auto &v = j->type == dJointTypeContact ? j->world->joints : j->world->arts;
        v.erase(std::remove(v.begin(), v.end(), j), v.end());
        if (j->type != dJointTypeContact) j->world->art_dirty = true;
        if (j->fb) j->world->n_feedback--;
    }
    if (j->group) { auto &v = j->group->joints; v.erase(std::remove(v.begin(), v.end(), j), v.end()); }
    delete j;
}
extern "C" void dJointSetFeedback(dJointID j, dJointFeedback *f)
{
    if (!j) return;
    if (j->world) j->world->n_feedback += (f ? 1 : 0) - (j->fb ? 1 : 0);
    j->fb = f;
}
extern "C" dJointFeedback *dJointGetFeedback(dJointID j) { return j ? j->fb : nullptr; }
extern "C" int dJointGetType(dJointID j) { return j ? j->type : dJointTypeNone; }
extern "C" dBodyID dJointGetBody(dJointID j, int index) { return !j ? nullptr : index == 0 ? j->b1 : index == 1 ? j->b2 : nullptr; }
extern "C" void dJointSetBallAnchor(dJointID j, dReal x, dReal y, dReal z) { if (j && j->type == dJointTypeBall) set_anchor(j, x, y, z); }
extern "C" void dJointGetBallAnchor(dJointID j, dVector3 r) { get_anchor(j, 0, r); }
extern "C" void dJointGetBallAnchor2(dJointID j, dVector3 r) { get_anchor(j, 1, r); }
extern "C" void dJointSetHingeAnchor(dJointID j, dReal x, dReal y, dReal z) { if (j && j->type == dJointTypeHinge) set_anchor(j, x, y, z); }
extern "C" void dJointGetHingeAnchor(dJointID j, dVector3 r) { get_anchor(j, 0, r); }
extern "C" void dJointGetHingeAnchor2(dJointID j, dVector3 r) { get_anchor(j, 1, r); }
extern "C" void dJointSetHingeAxis(dJointID j, dReal x, dReal y, dReal z)
{
    if (!j || j->type != dJointTypeHinge) return;
    const double l = sqrt((double)x * x + (double)y * y + (double)z * z);
    if (!(l > 0)) return;
    if (j->world) j->world->to_host();
    const double a[3] = { x / l, y / l, z / l };
    to_body(j->b1, a, false, j->axis1);
    to_body(j->b2, a, false, j->axis2);
    take_zero_pose(j);
    if (j->world) j->world->art_dirty = true;
}
extern "C" void dJointGetHingeAxis(dJointID j, dVector3 r)
{
    if (!j) return;
    if (j->world) j->world->to_host();
    to_world(j->b1, j->axis1, false, r);
}
// ---- a hinge's limit, motor, angle and rate.  dParamLoStop / HiStop / Vel / FMax are honoured (include/dmx_batch.h,
// dmxBatchSetHingeLimots: fudge factor 1, no bounce, the world's ERP / CFM at the stops); the other parameters say so once each
// call and are ignored.
static void set_limot_param(dJointID j, const char *fn, int parameter, dReal value)
{
    const double v = (double)value;
    const bool finite = v > -__builtin_huge_val() && v < __builtin_huge_val();
    switch (parameter) {
    case dParamLoStop: case dParamHiStop:
        if (v != v) { fprintf(stderr, "libode_mi355: %s: a stop that is not a number; ignored\n", fn); return; }
        (parameter == dParamLoStop ? j->lo_stop : j->hi_stop) = v;
        break;
    case dParamVel: case dParamFMax:
        if (!finite) { fprintf(stderr, "libode_mi355: %s: dParamVel / dParamFMax must be finite; ignored\n", fn); return; }
        (parameter == dParamVel ? j->vel : j->fmax) = v;
        break;
    default:
        fprintf(stderr, "libode_mi355: %s: parameter %d is not supported (dParamLoStop, HiStop, Vel, FMax are); ignored\n", fn, parameter);
        return;
    }
    if (j->world) j->world->limot_dirty = true;
}
static dReal get_limot_param(const dxJoint *j, int parameter)
{
    switch (parameter) {
    case dParamLoStop: return (dReal)j->lo_stop;
    case dParamHiStop: return (dReal)j->hi_stop;
    case dParamVel: return (dReal)j->vel;
    case dParamFMax: return (dReal)j->fmax;
    default: return 0;
    }
}
extern "C" void dJointSetHingeParam(dJointID j, int parameter, dReal value)
{
    if (j && j->type == dJointTypeHinge) set_limot_param(j, "dJointSetHingeParam", parameter, value);
}
extern "C" dReal dJointGetHingeParam(dJointID j, int parameter) { return j && j->type == dJointTypeHinge ? get_limot_param(j, parameter) : 0; }
// the hinge axis of the sides as attached, in the world frame: u = R_1 axis1
static void given_axis(const dxJoint *j, double u[3])
{
    dReal r[4];
    if (j->rev) to_world(nullptr, j->axis2, false, r); else to_world(j->b1, j->axis1, false, r);
    for (int k = 0; k < 3; k++) u[k] = (double)r[k];
}
extern "C" dReal dJointGetHingeAngle(dJointID j)
{
    if (!j || j->type != dJointTypeHinge || !j->b1) return 0;
    if (j->world) j->world->to_host();
    const dxBody *g1, *g2;
    dmx::Q4<double> q1, q2;
    given_sides(j, g1, g2, q1, q2);
    const double *ax = j->rev ? j->axis2 : j->axis1;
    const dmx::Q4<double> q0 = { j->qrel0[0], j->qrel0[1], j->qrel0[2], j->qrel0[3] };
    const dmx::V3<double> axis1 = { ax[0], ax[1], ax[2] };
    return (dReal)dmx::hinge_angle(q1, q2, q0, axis1);
}
extern "C" dReal dJointGetHingeAngleRate(dJointID j)
{
    if (!j || j->type != dJointTypeHinge || !j->b1) return 0;
    if (j->world) j->world->to_host();
    const dxBody *g1, *g2;
    dmx::Q4<double> q1, q2;
    given_sides(j, g1, g2, q1, q2);
    double u[3], d[3];
    given_axis(j, u);
    for (int k = 0; k < 3; k++) d[k] = (g1 ? (double)g1->avel[k] : 0.0) - (g2 ? (double)g2->avel[k] : 0.0);
    return (dReal)(u[0] * d[0] + u[1] * d[1] + u[2] * d[2]);
}
// +t u on body 1 and -t u on body 2 (the sides as attached), through the bodies' torque accumulators
extern "C" void dJointAddHingeTorque(dJointID j, dReal torque)
{
    if (!j || j->type != dJointTypeHinge || !j->b1) return;
    if (j->world) j->world->to_host();
    const dxBody *g1, *g2;
    dmx::Q4<double> q1, q2;
    given_sides(j, g1, g2, q1, q2);
    double u[3];
    given_axis(j, u);
    const double t = (double)torque;
    if (g1) dBodyAddTorque(const_cast<dxBody *>(g1), (dReal)(t * u[0]), (dReal)(t * u[1]), (dReal)(t * u[2]));
    if (g2) dBodyAddTorque(const_cast<dxBody *>(g2), (dReal)(-t * u[0]), (dReal)(-t * u[1]), (dReal)(-t * u[2]));
}
// ---- slider and fixed joints (include/dmx_batch.h, DMX_JOINT_SLIDER / DMX_JOINT_FIXED).  A slider's position, rate, stops, motor
// and dJointAddSliderForce are those of the sides as attached, as a hinge's angle is.
extern "C" dJointID dJointCreateSlider(dWorldID w, dJointGroupID g) { return create_art(w, g, dJointTypeSlider); }
extern "C" dJointID dJointCreateFixed(dWorldID w, dJointGroupID g) { return create_art(w, g, dJointTypeFixed); }
// the axis in world coordinates; the anchor is body 1's centre (body 2's when body 1 is the world: after the exchange that is
// dJointGetBody(j, 0) either way); this pose is the zero pose and s = 0
extern "C" void dJointSetSliderAxis(dJointID j, dReal x, dReal y, dReal z)
{
    if (!j || j->type != dJointTypeSlider) return;
    const double l = sqrt((double)x * x + (double)y * y + (double)z * z);
    if (!(l > 0)) return;
    if (j->world) j->world->to_host();
    const double a[3] = { x / l, y / l, z / l };
    to_body(j->b1, a, false, j->axis1);
    to_body(j->b2, a, false, j->axis2);
    const double p[3] = { j->b1 ? (double)j->b1->pos[0] : 0.0, j->b1 ? (double)j->b1->pos[1] : 0.0, j->b1 ? (double)j->b1->pos[2] : 0.0 };
    to_body(j->b1, p, true, j->anchor1);
    to_body(j->b2, p, true, j->anchor2);
    take_zero_pose(j);
    if (j->world) j->world->art_dirty = true;
}
extern "C" void dJointGetSliderAxis(dJointID j, dVector3 r)
{
    if (!j) return;
    if (j->world) j->world->to_host();
    to_world(j->b1, j->axis1, false, r);
}
extern "C" void dJointSetSliderParam(dJointID j, int parameter, dReal value)
{
    if (j && j->type == dJointTypeSlider) set_limot_param(j, "dJointSetSliderParam", parameter, value);
}
extern "C" dReal dJointGetSliderParam(dJointID j, int parameter) { return j && j->type == dJointTypeSlider ? get_limot_param(j, parameter) : 0; }
// s and s_dot of the sides as attached, through the function the device's position kernel and limot row use (slider_position)
static void slider_state(const dxJoint *j, double &s, double &s_dot)
{
    const dxBody *g1, *g2;
    dmx::Q4<double> q1, q2;
    given_sides(j, g1, g2, q1, q2);
    auto v3 = [](const dReal *p) -> dmx::V3<double> { return { (double)p[0], (double)p[1], (double)p[2] }; };
    auto d3 = [](const double *p) -> dmx::V3<double> { return { p[0], p[1], p[2] }; };
    const dmx::V3<double> zero = { 0.0, 0.0, 0.0 };
    dmx::slider_position<double>(g1 != nullptr, g1 ? v3(g1->pos) : zero, q1, g1 ? v3(g1->lvel) : zero, g1 ? v3(g1->avel) : zero,
                                 g2 != nullptr, g2 ? v3(g2->pos) : zero, q2, g2 ? v3(g2->lvel) : zero, g2 ? v3(g2->avel) : zero,
                                 d3(j->rev ? j->anchor2 : j->anchor1), d3(j->rev ? j->anchor1 : j->anchor2), d3(j->rev ? j->axis2 : j->axis1), s, s_dot);
}
extern "C" dReal dJointGetSliderPosition(dJointID j)
{
    if (!j || j->type != dJointTypeSlider || !j->b1) return 0;
    if (j->world) j->world->to_host();
    double s, sd;
    slider_state(j, s, sd);
    return (dReal)s;
}
extern "C" dReal dJointGetSliderPositionRate(dJointID j)
{
    if (!j || j->type != dJointTypeSlider || !j->b1) return 0;
    if (j->world) j->world->to_host();
    double s, sd;
    slider_state(j, s, sd);
    return (dReal)sd;
}
// +f u on body 1 and -f u on body 2 (the sides as attached), both at p_2: the limot row's J^T f, so the pair's momentum and angular
// momentum are untouched
extern "C" void dJointAddSliderForce(dJointID j, dReal force)
{
    if (!j || j->type != dJointTypeSlider || !j->b1) return;
    if (j->world) j->world->to_host();
    const dxBody *g1, *g2;
    dmx::Q4<double> q1, q2;
    given_sides(j, g1, g2, q1, q2);
    double u[3];
    given_axis(j, u);
    dReal p2[4];
    to_world(g2, j->rev ? j->anchor1 : j->anchor2, true, p2);
    for (int side = 0; side < 2; side++) {
        dxBody *b = const_cast<dxBody *>(side ? g2 : g1);
        if (!b) continue;
        const double f = side ? -(double)force : (double)force;
        const double r[3] = { (double)p2[0] - (double)b->pos[0], (double)p2[1] - (double)b->pos[1], (double)p2[2] - (double)b->pos[2] };
        dBodyAddForce(b, (dReal)(f * u[0]), (dReal)(f * u[1]), (dReal)(f * u[2]));
        dBodyAddTorque(b, (dReal)(f * (r[1] * u[2] - r[2] * u[1])), (dReal)(f * (r[2] * u[0] - r[0] * u[2])), (dReal)(f * (r[0] * u[1] - r[1] * u[0])));
    }
}
// welds the two bodies as they are now: the anchor at body 2's centre (body 1's when body 2 is the world), this pose the zero pose
extern "C" void dJointSetFixed(dJointID j)
{
    if (!j || j->type != dJointTypeFixed) return;
    if (j->world) j->world->to_host();
    const dxBody *c = (!j->rev && j->b2) ? j->b2 : j->b1;
    set_anchor(j, c ? c->pos[0] : 0, c ? c->pos[1] : 0, c ? c->pos[2] : 0);
}
// is there a joint between the two bodies (dAreConnectedExcluding: one whose type is not joint_type)?
extern "C" int dAreConnectedExcluding(dBodyID b1, dBodyID b2, int joint_type)
{
    if (!b1 || !b2 || b1->world != b2->world) return 0;
    const dxWorld *w = b1->world;
    for (const std::vector<dxJoint *> *v : { &w->arts, &w->joints })
        for (const dxJoint *j : *v)
            if (j->type != joint_type && ((j->b1 == b1 && j->b2 == b2) || (j->b1 == b2 && j->b2 == b1))) return 1;
    return 0;
}
// ---- angular motors (include/dmx_batch.h, DMX_JOINT_AMOTOR).  Axes, angles, rates, stops, motors and dJointAddAMotorTorques are those
// of the sides as attached, as a hinge's angle is: rel 1 / 2 name the body attached first / second, also after dJointAttach(j, 0, body).
namespace {

inline bool is_amotor(const dxJoint *j) { return j && j->type == dJointTypeAMotor; }
void amotor_touch(dJointID j) { if (j->world) j->world->amotor_dirty = true; }
// the body of the side `rel` names (1 / 2, the sides as attached; 0 or a world side: none)
const dxBody *amotor_side(const dxJoint *j, int rel)
{
    const dxBody *g1 = j->rev ? nullptr : j->b1, *g2 = j->rev ? j->b1 : j->b2;
    return rel == 1 ? g1 : rel == 2 ? g2 : nullptr;
}
// axes and angles of the sides as attached from the host mirrors, through the function the device uses
void amotor_now(const dxJoint *j, dmx::V3<double> a[3], double th[3])
{
    const dxBody *g1, *g2;
    dmx::Q4<double> q1, q2;
    given_sides(j, g1, g2, q1, q2);
    dmxAMotor m = j->am;
    if (m.num_axes < 1) m.num_axes = 1;
    dmx::amotor_axes<double>(g1 != nullptr, q1, g2 != nullptr, q2, m, a, th);
    if (j->am.num_axes < 1) { a[0] = { 0, 0, 0 }; th[0] = 0; }
}
// Euler mode: axis 0 goes with side 1 and axis 2 with side 2 whatever rel the caller gave, and "this pose is angles zero" -- the
// reference vectors -- is taken whenever axis 0 or 2 is set while both are known [ODE-recall amotorSetEulerReferenceVectors]
void amotor_euler_refs(dJointID j)
{
    dmxAMotor &m = j->am;
    if (m.mode != DMX_AMOTOR_EULER) return;
    m.num_axes = 3;
    dReal w0[4] = { 0, 0, 0, 0 }, w2[4] = { 0, 0, 0, 0 };
    to_world(amotor_side(j, m.rel[0]), m.axis[0], false, w0);
    to_world(amotor_side(j, m.rel[2]), m.axis[2], false, w2);
    const double a0[3] = { (double)w0[0], (double)w0[1], (double)w0[2] }, a2[3] = { (double)w2[0], (double)w2[1], (double)w2[2] };
    m.rel[0] = 1; m.rel[1] = 0; m.rel[2] = 2;
    to_body(amotor_side(j, 1), a0, false, m.axis[0]);
    to_body(amotor_side(j, 2), a2, false, m.axis[2]);
    if ((j->am_set & 5) == 5) {
        to_body(amotor_side(j, 1), a2, false, m.ref1);
        to_body(amotor_side(j, 2), a0, false, m.ref2);
    }
}

}  // namespace

extern "C" dJointID dJointCreateAMotor(dWorldID w, dJointGroupID g)
{
    dJointID j = create_art(w, g, dJointTypeAMotor);
    if (!j) return j;
    j->am.mode = DMX_AMOTOR_USER;
    for (int i = 0; i < 3; i++) { j->am.lo_stop[i] = -__builtin_huge_val(); j->am.hi_stop[i] = __builtin_huge_val(); }
    amotor_touch(j);
    return j;
}
extern "C" void dJointSetAMotorMode(dJointID j, int mode)
{
    if (!is_amotor(j) || (mode != dAMotorUser && mode != dAMotorEuler)) return;
    if (j->world) j->world->to_host();
    j->am.mode = mode == dAMotorEuler ? DMX_AMOTOR_EULER : DMX_AMOTOR_USER;
    amotor_euler_refs(j);
    amotor_touch(j);
}
extern "C" int dJointGetAMotorMode(dJointID j) { return is_amotor(j) && j->am.mode == DMX_AMOTOR_EULER ? dAMotorEuler : dAMotorUser; }
extern "C" void dJointSetAMotorNumAxes(dJointID j, int num)
{
    if (!is_amotor(j)) return;
    j->am.num_axes = j->am.mode == DMX_AMOTOR_EULER ? 3 : num < 0 ? 0 : num > 3 ? 3 : num;
    amotor_touch(j);
}
extern "C" int dJointGetAMotorNumAxes(dJointID j) { return is_amotor(j) ? j->am.num_axes : 0; }
extern "C" void dJointSetAMotorAxis(dJointID j, int anum, int rel, dReal x, dReal y, dReal z)
{
    if (!is_amotor(j) || anum < 0 || anum > 2 || rel < 0 || rel > 2) return;
    const double l = sqrt((double)x * x + (double)y * y + (double)z * z);
    if (!(l > 0) || !(l < __builtin_huge_val())) return;
    if (j->world) j->world->to_host();
    const double a[3] = { x / l, y / l, z / l };
    j->am.rel[anum] = rel;
    to_body(amotor_side(j, rel), a, false, j->am.axis[anum]);
    j->am_set |= 1 << anum;
    amotor_euler_refs(j);
    amotor_touch(j);
}
extern "C" void dJointGetAMotorAxis(dJointID j, int anum, dVector3 r)
{
    if (!is_amotor(j) || anum < 0 || anum > 2) return;
    if (j->world) j->world->to_host();
    if (j->am.mode == DMX_AMOTOR_EULER) {
        dmx::V3<double> a[3];
        double th[3];
        amotor_now(j, a, th);
        r[0] = (dReal)a[anum].x; r[1] = (dReal)a[anum].y; r[2] = (dReal)a[anum].z;
        return;
    }
    to_world(amotor_side(j, j->am.rel[anum]), j->am.axis[anum], false, r);
}
extern "C" int dJointGetAMotorAxisRel(dJointID j, int anum) { return is_amotor(j) && anum >= 0 && anum <= 2 ? j->am.rel[anum] : 0; }
extern "C" void dJointSetAMotorAngle(dJointID j, int anum, dReal angle)
{
    if (!is_amotor(j) || anum < 0 || anum > 2) return;
    const double v = (double)angle;
    if (!(v > -__builtin_huge_val() && v < __builtin_huge_val())) { fprintf(stderr, "libode_mi355: dJointSetAMotorAngle: an angle that is not finite; ignored\n"); return; }
    if (j->am.mode != DMX_AMOTOR_USER) return;       // (Euler mode computes its angles)
    j->am.angle[anum] = v;
    amotor_touch(j);
}
extern "C" dReal dJointGetAMotorAngle(dJointID j, int anum)
{
    if (!is_amotor(j) || anum < 0 || anum > 2) return 0;
    if (j->am.mode == DMX_AMOTOR_USER) return (dReal)j->am.angle[anum];
    if (j->world) j->world->to_host();
    dmx::V3<double> a[3];
    double th[3];
    amotor_now(j, a, th);
    return (dReal)th[anum];
}
// a_i . (omega_1 - omega_2) of the sides as attached: the velocity axis i's row acts on (include/dmx_batch.h, "rate")
extern "C" dReal dJointGetAMotorAngleRate(dJointID j, int anum)
{
    if (!is_amotor(j) || anum < 0 || anum > 2 || anum >= j->am.num_axes) return 0;
    if (j->world) j->world->to_host();
    dmx::V3<double> a[3];
    double th[3];
    amotor_now(j, a, th);
    const dxBody *g1 = amotor_side(j, 1), *g2 = amotor_side(j, 2);
    double d[3];
    for (int k = 0; k < 3; k++) d[k] = (g1 ? (double)g1->avel[k] : 0.0) - (g2 ? (double)g2->avel[k] : 0.0);
    return (dReal)(a[anum].x * d[0] + a[anum].y * d[1] + a[anum].z * d[2]);
}
// dParamLoStop / HiStop / Vel / FMax and their ...2 / ...3 groups are honoured (fudge factor 1, no bounce, the world's ERP / CFM at the
// stops); the other parameters say so once each call and are ignored
extern "C" void dJointSetAMotorParam(dJointID j, int parameter, dReal value)
{
    if (!is_amotor(j)) return;
    const int i = parameter / dParamGroup, base = parameter % dParamGroup;
    const double v = (double)value;
    const bool finite = v > -__builtin_huge_val() && v < __builtin_huge_val();
    if (parameter < 0 || i > 2) { fprintf(stderr, "libode_mi355: dJointSetAMotorParam: parameter %d is not supported; ignored\n", parameter); return; }
    switch (base) {
    case dParamLoStop: case dParamHiStop:
        if (v != v) { fprintf(stderr, "libode_mi355: dJointSetAMotorParam: a stop that is not a number; ignored\n"); return; }
        (base == dParamLoStop ? j->am.lo_stop : j->am.hi_stop)[i] = v;
        break;
    case dParamVel: case dParamFMax:
        if (!finite) { fprintf(stderr, "libode_mi355: dJointSetAMotorParam: dParamVel / dParamFMax must be finite; ignored\n"); return; }
        (base == dParamVel ? j->am.vel : j->am.fmax)[i] = v;
        break;
    default:
        fprintf(stderr, "libode_mi355: dJointSetAMotorParam: parameter %d is not supported (dParamLoStop, HiStop, Vel, FMax and their groups are); ignored\n", parameter);
        return;
    }
    amotor_touch(j);
}
extern "C" dReal dJointGetAMotorParam(dJointID j, int parameter)
{
    if (!is_amotor(j) || parameter < 0 || parameter / dParamGroup > 2) return 0;
    const int i = parameter / dParamGroup;
    switch (parameter % dParamGroup) {
    case dParamLoStop: return (dReal)j->am.lo_stop[i];
    case dParamHiStop: return (dReal)j->am.hi_stop[i];
    case dParamVel: return (dReal)j->am.vel[i];
    case dParamFMax: return (dReal)j->am.fmax[i];
    default: return 0;
    }
}
// +sum t_i a_i on body 1 and the opposite on body 2 (the sides as attached), through the bodies' torque accumulators
extern "C" void dJointAddAMotorTorques(dJointID j, dReal torque1, dReal torque2, dReal torque3)
{
    if (!is_amotor(j) || !j->b1) return;
    if (j->world) j->world->to_host();
    dmx::V3<double> a[3];
    double th[3];
    amotor_now(j, a, th);
    const double t[3] = { (double)torque1, (double)torque2, (double)torque3 };
    double s[3] = { 0, 0, 0 };
    for (int i = 0; i < j->am.num_axes && i < 3; i++) { s[0] += t[i] * a[i].x; s[1] += t[i] * a[i].y; s[2] += t[i] * a[i].z; }
    const dxBody *g1 = amotor_side(j, 1), *g2 = amotor_side(j, 2);
    if (g1) dBodyAddTorque(const_cast<dxBody *>(g1), (dReal)s[0], (dReal)s[1], (dReal)s[2]);
    if (g2) dBodyAddTorque(const_cast<dxBody *>(g2), (dReal)-s[0], (dReal)-s[1], (dReal)-s[2]);
}

extern "C" int dAreConnected(dBodyID b1, dBodyID b2) { return dAreConnectedExcluding(b1, b2, dJointTypeNone); }

// ================================================================================ rotation helpers
extern "C" void dRSetIdentity(dMatrix3 R) { set_identity(R); }
extern "C" void dQtoR(const dQuaternion q, dMatrix3 R) { from_m3(dmx::quat_to_R(Q4<dReal>{ q[0], q[1], q[2], q[3] }), R); }
extern "C" void dRtoQ(const dMatrix3 R, dQuaternion q)
{
    const Q4<dReal> r = dmx::R_to_quat(to_m3(R));
    q[0] = r.w; q[1] = r.x; q[2] = r.y; q[3] = r.z;
}
extern "C" void dRFromAxisAndAngle(dMatrix3 R, dReal ax, dReal ay, dReal az, dReal angle)
{
    dReal l = ax * ax + ay * ay + az * az;
    Q4<dReal> q = { 1, 0, 0, 0 };
    if (l > 0) {
        angle *= (dReal)0.5;
        l = (dReal)sin((double)angle) / dmx::tsqrt<dReal>(l);
        q = { (dReal)cos((double)angle), ax * l, ay * l, az * l };
    }
    from_m3(dmx::quat_to_R(q), R);
}

// ================================================================================ snapshot extension
extern "C" int dmxWorldSnapshotTransforms(dWorldID w, const dBodyID *bodies, int n, dReal *out)
{
    if (!w || !bodies || !out || n < 0) return 0;
    w->to_device();
    w->buf.resize((size_t)w->cap * 16);
    DMX_MUST(dmxBatchDownloadTransforms(w->batch, w->buf.data(), 0, w->cap));
    for (int i = 0; i < n; i++) {
        if (!bodies[i] || bodies[i]->world != w) return 0;
        memcpy(out + (size_t)i * 16, w->buf.data() + (size_t)bodies[i]->slot * 16, 16 * sizeof(dReal));
    }
    return 1;
}

// The whole of main.c:221-237 in one call: walks the caller's array of body handles (stride body_stride bytes, as in
// `Body bodies[MAX_BODIES]`, body.h:20-24) and writes each live body's column-major 4x4 into the caller's array of
// states (stride state_stride bytes, as in `BodyState bodyStates[MAX_BODIES]`, body.h:26-31).  Entries whose handle is
// 0 (empty slots, static geoms: main.c:228) are left untouched.  Returns the number of transforms written, -1 on error.
extern "C" int dmxWorldSnapshotBodyStates(dWorldID w, const void *first_body, size_t body_stride, int n,
                                          void *first_transform, size_t state_stride)
{
    if (!w || !first_body || !first_transform || n < 0 || body_stride < sizeof(dBodyID) || state_stride < 16 * sizeof(dReal))
        return -1;
    w->to_device();
    w->buf.resize((size_t)w->cap * 16);
    DMX_MUST(dmxBatchDownloadTransforms(w->batch, w->buf.data(), 0, w->cap));
    int written = 0;
    for (int i = 0; i < n; i++) {
        dBodyID b;
        memcpy(&b, (const char *)first_body + (size_t)i * body_stride, sizeof b);
        if (!b) continue;
        if (b->world != w) return -1;
        memcpy((char *)first_transform + (size_t)i * state_stride, w->buf.data() + (size_t)b->slot * 16, 16 * sizeof(dReal));
        written++;
    }
    return written;
}
