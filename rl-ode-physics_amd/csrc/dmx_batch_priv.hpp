// dmx_batch_priv.hpp -- the batch object behind dmxBatchID, shared by the C-ABI translation units.
#pragma once

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <algorithm>
#include <chrono>
#include <functional>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/dmx_batch.h"
#include "dmx_internal.hpp"
#include "dmx_uniform.hpp"
#include "dmx_fixed.hpp"
#include "dmx_autodisable.hpp"
#include "dmx_damping.hpp"
#include "dmx_amotor.hpp"

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            fprintf(stderr, "libode_mi355: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), \
                    __FILE__, __LINE__);                                                           \
            return DMX_EHIP;                                                                       \
        }                                                                                          \
    } while (0)

using namespace dmx;

// a contact joint in canonical form: body1 a live dynamic slot, normal into it (dmx_joints.cpp)
// ... or a unit of an articulation joint (unit != 0: j is null, art = its index in the batch's set): at most three rows on the
// same two bodies, carried beside the contacts -- a ball is one DMX_UNIT_BALL, a hinge a DMX_UNIT_BALL and a DMX_UNIT_HINGE2
// and, when its limot is present (dmxBatchSetHingeLimots), a UNIT_LIMOT of one row; a slider a UNIT_LOCK, a UNIT_SLIDER2 and, when
// present, a UNIT_SLIMOT; a fixed joint a UNIT_BALL and a UNIT_LOCK.  An angular motor is one UNIT_AMOTOR
// of one row per axis whose limot is present (dmxBatchSetAMotors).  The two limot units and UNIT_AMOTOR are the only ones whose row can clamp
struct DmxCanonicalJoint { int b1, b2; const dmxContactJoint *j; bool rev; int unit = 0; int art = -1; int axis = 0; };      // (axis: a UNIT_AMOTOR's)

struct dmxBatch {
    int64_t n = 0, stride = 0;
    void *pack_out = nullptr; int64_t pack_lo = 0, pack_hi = 0;   // dmxBatchSetBoundaryPack
    int64_t n_active = 0;            // bodies [0, n_active) are stepped; the rest are ghost slots
    int precision = DMX_F32;
    int device = 0;
    size_t rsize = 4;
    void *slab = nullptr;            // C_COUNT x stride reals: the CURRENT slab (state, constants, zones)
    // Second slab of the same layout.  Constants and zones are kept identical in both (every writer of those
    // components writes both); the state lives in `slab`.  The first launch of a collision-proof chunk reads `slab`
    // and writes the new state to `slab_alt`, then the two swap roles: the chunk's start state stays behind,
    // untouched, as the rollback snapshot (rollback = swap back) at no copy and no extra traffic.
    void *slab_alt = nullptr;
    bool flip_armed = false;         // the next fast launch starts a chunk: write out of place and swap
    bool flipped = false;            // this chunk has swapped: its snapshot is `slab_alt`
    // The direction in which the next contact-free launch walks the tiles (dmx_sweep.hpp); flipped after every such launch, the
    // out-of-place first launch of a chunk included (the lines it wrote into the other slab are what the next tick reads).
    // Any direction is correct, so a rollback or a rebuilt chunk needs no care; a launch recorded into a HIP graph bakes its
    // direction in -- the replays of one recording alternate among themselves as recorded, and whatever the neighbours do is correct.
    bool sweep_rev = false;
    int snapshot_mode = DMX_SNAPSHOT_PINGPONG;
    int snap_kind = 0;               // how the chunk in flight keeps its start state (dmx_general.cpp: SNAP_*)
    // a collision-proof chunk left open by dmxBatchStep (dmx_general.cpp "lazy chunks"): its calls so far, to replay
    // them after a rollback; closed by dmx_settle
    struct OpenChunk {
        bool open = false, ballistic = false, last_checked = false;
        int ticks = 0, budget = 0;
        std::vector<std::pair<double, int>> segs;       // (h, ticks) per Step call, in order
    } oc;
    bool lazy_chunks = true;         // DMX_LAZY_CHUNKS=0 reads every chunk's flag before dmxBatchStep returns
    uint8_t *gtype = nullptr;        // stride bytes
    StepDiag *diag = nullptr;        // device, one slot per wave of the fused step
    StepDiag *diag_isl = nullptr;    // device, island path (atomics)
    size_t n_diag = 0;
    bool last_islands = false;       // which diagnostics the last tick wrote
    StepDiag *diag_host = nullptr;   // pinned
    void *stage = nullptr;           // device staging between host-order rows and the tiled slab
    size_t stage_bytes = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    // an exact tick's fused step for the bodies outside the islands runs beside the island solve (disjoint bodies): a second
    // stream forked from `stream` after the tick's record and joined behind the solve (dmx_general.cpp: careful_tick)
    hipStream_t fork_stream = nullptr; hipEvent_t fork_ev = nullptr, join_ev = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // world parameters (defaults: dWorldCreate [ODE], gravity unset = 0)
    double g[3] = { 0, 0, 0 };
    double erp = 0.2, cfm = 1e-5, sor_w = 1.3;
    int iters = 20;
    int gyro = DMX_GYRO_IMPLICIT;
    int plane_on = 0;
    double plane[4] = { 0, 1, 0, 0 };
    int surf_mode = DMX_CONTACT_BOUNCE;                 // main.c:684
    double mu = __builtin_huge_val(), bounce = 0.2, bounce_vel = 0.1;   // main.c:685-687
    int max_contacts = 8;                               // main.c:675
    bool ext_pending = false;
    // host scratch of the island grouping, persistent between ticks (dmx_joints.cpp) and of the exact tick (dmx_general.cpp)
    std::vector<int> sc_parent, sc_island, sc_last, sc_slots;
    std::vector<int> sc_iv[16];                 // work arrays of the island grouping (dmx_joints.cpp)
    std::vector<DmxCanonicalJoint> sc_cj;
    std::vector<uint8_t> sc_include;            // per slot: 1 while the body is in this tick's island subset
    const int32_t *sc_include_list = nullptr;   // that subset as an ascending list (set around dmx_step_joints by the exact tick)
    int64_t sc_include_count = 0;
    // host-side phase timers of the exact tick (seconds), printed at destroy when DMX_HOST_PROFILE is set
    double prof[12] = { 0 }; bool prof_on = false;
    int ticks_per_launch = 1;        // contact-free ticks fused into one integrate_free launch (dmxBatchSetTicksPerLaunch)
    // integrate_free's removals (dmxBatchSetElision; DMX_ELIDE in the environment sets the default): bit 0 = store elision,
    // bit 1 = uniform mass / inertia as kernel arguments.  The trackers follow every upload of the two fields (upload_t).
    int elide = DMX_ELIDE_STORES | DMX_ELIDE_CONSTANTS;
    dmx::UniformTracker<1> uni_mass; dmx::UniformTracker<3> uni_inertia;
    bool capturing = false;          // the stream was being captured into a HIP graph at the last stepping call (dmx_note_capture)
    // integrate_free's third removal (dmxBatchSetLoadElision; DMX_ELIDE_LOADS=0 in the environment switches it off): loads of
    // pos.x/z and lvel.x/z in tiles that have proven them fixed.  fix_words: one word per 64-body tile, on the device, bits 0..2 =
    // axis x, y, z fixed; `fix` says before each contact-free launch whether the words may be used (dmx_fixed.hpp has the rule).
    dmx::FixedChain fix;
    uint32_t *fix_words = nullptr;   // stride / 64 words
    // integrate_free's short tick of a body without torque (dmxBatchSetTorqueFree; DMX_TORQUE_FREE=0 in the environment switches it
    // off): dmx_torque_free.hpp decides per launch whether it applies.  Off, the launches are the ones they always were.
    bool torque_free = true;
    int64_t tf_stats[2] = { 0, 0 };  // contact-free launches with / without the short tick built in (dmxBatchTorqueFreeStats)
    // integrate_free_lean, the straight-line kernel of a lean launch (dmxBatchSetLeanKernel; DMX_LEAN_KERNEL=0 in the environment
    // switches it off): launch_step decides per launch whether it applies.  Off, the launches are the ones they always were.
    bool lean_kernel = true;
    int64_t lk_stats[2] = { 0, 0 };  // contact-free launches that took that kernel / that did not (dmxBatchLeanKernelStats)
    bool stepped_with_plane = false;
    // general island path (explicit contact joints)
    uint8_t *bflags = nullptr;                 // device, per-slot BF_* flags
    std::vector<uint8_t> h_bflags;             // host mirror
    int64_t n_flagged = 0;                     // slots of [0, n_active) whose byte is not BF_ALIVE (dmx_refuse_flags)
    struct DevBuf { void *p = nullptr; size_t bytes = 0; };
    DevBuf jd_int, jd_real, jd_rows, jd_rowjb, jd_bscr, jd_local;   // device staging / scratch
    std::vector<int> sc_nbd_of, sc_grid_list; std::vector<std::pair<uint64_t, int>> sc_pair_ord;
    void *lcp_grid = nullptr;                  // dWorldStep's grid-wide solve of large islands (dmx_lcp.hip): buffers, remembered active sets
    double exs_acc[64] = { 0 }; long exs_ticks = 0;      // DMX_EXS_TIMING: stage times of the small-scene exact tick, summed
    void *ex_counts_dev = nullptr, *bp_flags_dev = nullptr;    // device-visible addresses of ex_counts_host / bp_flags_host
    int exact_pipeline = 0;         // dmxBatchSetExactPipeline (DMX_EXACT_*); the environment's DMX_SMALL_EXACT is the default
    bool bp_fresh = false;          // the safe zones were built at exactly the current poses (no tick since)
    bool snap_fresh = false;        // ... as of the open snapshot
    bool bp_skip_fast = false;      // the next chunk goes the exact way without trying the fast one (a retry would repeat a failure)
    bool stepper_exact = false;                // dmxBatchSetStepper: dmxBatchStepJoints solves every island's LCP exactly
    bool row_order_ode = false;                // dmxBatchSetRowOrder: ODE's joint-discovery row order + periodic LCG shuffle (QuickStep)
    uint32_t ode_rand = 0;                     // that LCG's state (ODE's is process-global; here it belongs to the batch)
    std::vector<int> sc_ode_proc, sc_ode_iv[4], sc_ode_order;
    std::vector<uint8_t> sc_ode_tag_b, sc_ode_tag_j;
    DevBuf jd_order;
    void *jh_int = nullptr, *jh_real = nullptr;                      // pinned host staging
    // body-body broadphase (dmx_broadphase.hip / dmx_general.cpp)
    int bp_enabled = 1;                        // dmxBatchSetBodyCollisions
    bool bp_valid = false;                     // safe zones match the current constant data
    int bp_chunk = 0;                          // current fast-chunk length in ticks (adaptive, dmx_general.cpp)
    uint32_t bp_crowded = 0;                   // bodies whose safe radius is <= 0 at the last build
    double bp_rmax = 0, bp_rcls[4] = { 0, 0, 0, 0 };
    uint32_t bp_mask = 0; int bp_cap = 8; int bp_xbits = -1;      // -1: not chosen yet
    DevBuf bp_count, bp_items, bp_flags, bp_inpair, bp_snapshot;
    // device-resident bookkeeping of the exact tick (dmx_exact.hip): capacity estimates carried from tick to tick, one arena
    // for the pipeline's arrays, per-body scan arrays, the per-slot level scratch, the pinned read-back record
    uint32_t ex_cap_pairs = 0, ex_cap_rows = 0;
    uint32_t ex_prev_inv = 1;                   // bodies the last exact tick found involved (in a pair / at a static box)
    DevBuf ex_arena, ex_body, ex_last, ex_aabb;
    void *ex_counts_host = nullptr;
    std::vector<int32_t> fp_pairs, fp_inv, fp_cross;      // dmxBatchFindPairs' results; (own body, ghost slot) pairs it met
    uint32_t *bp_flags_host = nullptr;         // pinned
    std::vector<double> h_sides;               // host mirror of DMX_SIDES (exact values of the batch precision)
    std::vector<uint8_t> h_gtype;
    // convex bodies: the shared hull's body-frame points, and the per-tick plane contacts of every convex body
    DevBuf hull, cbuf, ccount;
    DevBuf hull_planes; int hull_nf = 0;       // the hull's faces (dmxBatchSetConvexHullFaces): 4 reals each
    bool spec_refused = false;                 // the last exact tick's record refused (or would have refused) the speculative launches
    int64_t stat_spec_ticks = 0;               // exact ticks whose solve + fused step went out before the host had the counts, and stood
    int64_t stat_unsupported = 0;              // AABB pairs met that have no collider (convex-convex, convex-sphere)
    DevBuf sbox; int n_static = 0;             // static box geoms (dmxBatchSetStaticBoxes), SBOX_REALS reals each
    // the fused path of bodies at static geometry (np_static -> step_contacts): per-body contact buffer and counts
    DevBuf sbuf, scount;
    uint32_t class_pairs = CLASS_PAIRS_ALL;     // dmxBatchSetClassPairs: which geometry classes collide with which
    bool has_simple = true;                    // some slot is a box or a sphere (kept by dmxBatchUploadGeomType)
    int64_t n_simple = 0;                      // ... how many (h_gtype starts all GEOM_NONE)
    bool static_fast = true;                   // DMX_STATIC_FAST=0: every body at a static box goes through the exact tick (round 2's way)
    bool static_need8 = false;                 // a body with 5..8 static contacts has been met: the second step_contacts launch rides along
    int nofast_hold = 0, nofast_level = 0;     // chunks to go the exact way after a body overflowed the contact buffer (backs off)
    int hull_n = 0;
    int64_t stat_rollbacks = 0;
    int64_t stat_fast_ticks = 0, stat_careful_ticks = 0, stat_rebuilds = 0, stat_pair_ticks = 0;
    unsigned long long last_pairs = 0;
    bool last_mixed = false;                   // last tick used fused + island kernels together
    size_t jh_int_bytes = 0, jh_real_bytes = 0;
    // single-launch tick of small worlds (dmx_small.hip; the host side is in dmx_joints.cpp)
    int small_mode = DMX_SMALL_TICK_AUTO;          // dmxBatchSetSmallTick; DMX_SMALL_TICK=0 makes OFF the default
    int64_t small_stats[DMX_SMALL_TICK_NSTATS] = { 0 };
    // host-mapped pinned staging (ints, then reals), two buffers used alternately: tick k + 1's tables are filled while tick k's
    // kernel may still read its own; sm_ev[p] is recorded behind the launch that reads buffer p
    void *sm_stage[2] = { nullptr, nullptr }, *sm_stage_dev[2] = { nullptr, nullptr };
    size_t sm_stage_bytes[2] = { 0, 0 };
    hipEvent_t sm_ev[2] = { nullptr, nullptr }; bool sm_ev_pending[2] = { false, false };
    int sm_parity = 0;
    // the mirror: 13 reals per slot (DMX_STATE order), host-mapped pinned, written by small_world_tick.  Valid = it holds the
    // slab's state once the stream has drained; EVERY other writer of body state clears the flag (dmx_state_written)
    void *sm_mirror = nullptr, *sm_mirror_dev = nullptr;
    bool sm_mirror_valid = false;
    bool sm_lcp_touched = false;                   // dmx_touch_lcp done for this batch (first small dWorldStep tick)
    bool slab_exposed = false;                     // dmxBatchDevicePtr handed the slab out: writes the batch cannot see -- the mirror is never served
    StepDiag *sm_diag = nullptr; int sm_diag_cur = 0;      // two device slots used alternately (each launch zeroes the next one's)
    bool last_small = false;                       // the last dmxBatchStepJoints tick left its diagnostics in sm_diag[sm_diag_cur]
    // ray casts (dmx_general.cpp "ray casts", dmx_raycast.hip).  The column grid rays walk is a table of the ray cast's own --
    // same size and hashing as the broadphase's, its own bucket capacity and torus / scrambled choice -- so that a cast leaves
    // nothing behind that a tick could meet: not a grown bucket, not a cleared flag.  It is rebuilt when state_version has
    // moved on from the build's (every writer of poses, extents, classes or flags bumps it), or always once the slab's address
    // has been handed out (slab_exposed).
    uint64_t state_version = 1, rc_version = 0;
    int rc_cap = 8, rc_xbits = -1;                 // -1: not chosen yet
    double rc_rmax = 0;                            // the bounding radius the built grid's cell width came from
    int ray_form = 0;                              // dmxBatchSetRayForm; DMX_RAY_FORM in the environment sets the default
    DevBuf rc_count, rc_items, rc_misc;            // rc_misc: BPF_COUNT flag words, then the rectangle's four keys at byte 64
    DevBuf rc_rays, rc_ids, rc_hits;               // device staging of dmxBatchRayCast's host arrays
    // articulation joints (dmxBatchSetJoints): the set, and the device staging of dmxBatchJointErrors
    std::vector<dmxJoint> art;
    DevBuf art_dev, art_err;
    // the hinges' limits and motors (dmxBatchSetHingeLimots): empty, or one entry per joint of `art`
    std::vector<dmxHingeLimot> limot;
    DevBuf limot_dev;
    // the angular motors (dmxBatchSetAMotors): empty, or one entry per joint of `art`; amotor_in / amotor_prep: the device staging of
    // dmxBatchAMotorAngles' records and the table amotor_prepare writes (a tick's records travel with its own tables); am_rec: the
    // host's scratch for the records
    std::vector<dmxAMotor> amotor;
    DevBuf amotor_in, amotor_prep;
    std::vector<dmx::AMotorIn> am_rec;
    std::vector<char> am_tmp;                          // dmxBatchAMotorAngles' download
    std::vector<std::pair<int, int>> sc_am_links;      // the tick in the making: body pairs its active AMotors link (dmx_joints.cpp)
    // feedback (dmxBatchSetFeedback): fb_valid = the last tick was a dmxBatchStepJoints tick made with it on (every other writer of
    // body state clears it: dmx_state_stepped); 12 reals per result in the batch's precision, the set's joints first, then the
    // tick's contact joints: on the device at fb_devp -- fb_dev on the general path, behind a small tick's tables in its host-mapped
    // staging otherwise, where fb_host is the host's address of the same memory
    bool fb_on = false, fb_valid = false;
    int64_t fb_nj = 0, fb_nc = 0;
    DevBuf fb_dev;
    const void *fb_devp = nullptr, *fb_host = nullptr;
    std::vector<char> fb_tmp;
    int64_t last_units = 0;                        // units the last dmxBatchStepJoints tick carried among its contact entries
    // auto-disable (dmxBatchSetAutoDisable; the rule is in dmx_autodisable.hpp, the host side in dmx_joints.cpp).  The counters
    // live on the device, one per slot, allocated with the first slot that carries DMX_BODY_AUTODISABLE.  ad_mirror: one byte
    // per slot, host-mapped pinned -- a single-launch tick's kernel writes the stepped slots' flag bytes there, the general
    // path copies the device's flag bytes into it behind its kernels; ad_pending = such a tick is enqueued and its DISABLED bits
    // have not reached h_bflags yet: dmx_ad_merge waits for ad_ev (recorded behind the tick) and takes them over.
    double ad_lin = 0.01, ad_ang = 0.01, ad_time = 0.0;
    int ad_steps = 10;
    int32_t *ad_steps_dev = nullptr; double *ad_time_dev = nullptr;
    uint8_t *ad_mirror = nullptr, *ad_mirror_dev = nullptr;
    hipEvent_t ad_ev = nullptr, ad_wait_ev = nullptr; bool ad_pending = false;      // ad_wait_ev: ad_ev, or the small tick's own event
    int64_t ad_n_auto = 0, ad_n_disabled = 0;      // slots of [0, n) that carry AUTODISABLE / ALIVE and DISABLED, by h_bflags
    int64_t ad_skipped = 0, ad_slept = 0, ad_woken = 0, ad_flag_reads = 0;      // dmxBatchAutoDisableStats [1] .. [3]; dmxBatchDownloadBodyFlags calls
    std::vector<int> sc_ad_dropped;                // the live slots the tick in the making leaves out (asleep islands)
    std::vector<uint8_t> sc_awake;                 // per slot, idle = 0: the island rooted at the slot holds an awake body (dmx_joints.cpp)
    // damping, angular speed cap, contact correction (include/dmx_batch.h, "damping"; the rules are in dmx_damping.hpp and
    // contact_rows).  h_damp: the table as given, empty until a call sets a non-default value; damp_dev: the same on the device,
    // DAMP_REALS reals per slot of the stride in the batch's precision.  The three counts follow every change of the table
    // (dmx_damp_recount): entries of [0, n_active) that differ from the defaults (the refusal), slots of [0, n) with a scale
    // other than zero (the damping kernel is launched) and with a finite maximum speed (finish_body is handed the table).
    std::vector<dmxBodyDamping> h_damp;
    void *damp_dev = nullptr;
    int64_t damp_n_set = 0, damp_n_scaled = 0, damp_n_capped = 0;
    double surface_layer = 0.0, max_corr_vel = __builtin_huge_val();
};
void dmx_damp_recount(dmxBatch *b);
// the ticks that find their own contacts know neither damping, nor the angular speed cap, nor the contact correction scalars
inline bool dmx_refuse_stability(const dmxBatch *b, const char *what)
{
    const bool scalars = b->surface_layer != 0.0 || b->max_corr_vel != __builtin_huge_val();
    if (b->damp_n_set == 0 && !scalars) return false;
    fprintf(stderr, "libode_mi355: %s does not honour damping, the maximum angular speed or the contact correction scalars (dmxBatchSetDamping, "
                    "dmxBatchSetMaxAngularSpeed, dmxBatchUploadBodyDamping, dmxBatchSetContactCorrection): %lld slot(s) hold a non-default entry, "
                    "surface_layer = %g, max_correcting_vel = %g; use dmxBatchStepJoints\n",
            what, (long long)b->damp_n_set, b->surface_layer, b->max_corr_vel);
    return true;
}
// auto-disable: the per-slot counters (reset to the batch's values) and the flag mirror, made when the feature is first used
int dmx_ad_ensure(dmxBatch *b);
// the DISABLED bits a tick enqueued earlier has set -> h_bflags (waits for that tick; nothing to do when none is pending)
int dmx_ad_merge(dmxBatch *b);
inline bool dmx_limot_present(const dmxHingeLimot &l) { return dmx::limot_present(l.lo_stop, l.hi_stop, l.fmax); }
// amotor_prepare's records, one per joint of the set (dmx_artic.hip)
void dmx_amotor_records(const dmxBatch *b, dmx::AMotorIn *out);
// is axis i of an AMotor a row?  The hinge's rule, on the parameters alone
inline bool dmx_amotor_present(const dmxAMotor &m, int i) { return i < m.num_axes && dmx::limot_present(m.lo_stop[i], m.hi_stop[i], m.fmax[i]); }
// the ticks that build their own islands on the device do not know articulation joints: they say so instead of ignoring them
inline bool dmx_refuse_joints(const dmxBatch *b, const char *what)
{
    if (b->art.empty()) return false;
    fprintf(stderr, "libode_mi355: %s does not honour articulation joints (dmxBatchSetJoints): %lld are set; use dmxBatchStepJoints\n",
            what, (long long)b->art.size());
    return true;
}
// ... and neither do they know the per-body flags on their fast paths (the fused ticks never read them, the islands they hand to
// launch_islands do): a kinematic body would fall while alone and stand while touched.  They refuse too, from a count kept on
// the host by dmxBatchUploadBodyFlags and dmxBatchSetActiveCount; ghost slots do not count, nobody steps them
inline bool dmx_refuse_flags(const dmxBatch *b, const char *what)
{
    if (b->n_flagged == 0) return false;
    fprintf(stderr, "libode_mi355: %s does not honour per-body flags (dmxBatchUploadBodyFlags): %lld slot(s) carry a byte other than DMX_BODY_ALIVE (DMX_BODY_AUTODISABLE and DMX_BODY_DISABLED included); use dmxBatchStepJoints\n",
            what, (long long)b->n_flagged);
    return true;
}
// ... nor friction bounded by the normal force (DMX_CONTACT_APPROX1 in the batch surface, dmxBatchSetSurface): their fused kernels bound
// friction rows by mu newtons.  While the surface would make a pyramid row -- a bit set and 0 < mu < inf -- they refuse.
inline bool dmx_refuse_approx1(const dmxBatch *b, const char *what)
{
    if (!(b->surf_mode & DMX_CONTACT_APPROX1) || !(b->mu > 0 && b->mu < __builtin_huge_val())) return false;
    fprintf(stderr, "libode_mi355: %s does not honour friction bounded by the normal force (DMX_CONTACT_APPROX1 in dmxBatchSetSurface, mu = %g); use dmxBatchStepJoints\n",
            what, b->mu);
    return true;
}
// A launch recorded into a HIP graph would bake the uniform constants' VALUES in, and replays would keep them after a later
// upload of another mass while eager ticks use the new one: launches recorded during a capture read the constants from the
// slab.  Asked once per stepping call of the C ABI (the entry points that can reach integrate_free), not per tick.
// The fixed-axis words (dmx_fixed.hpp) cannot outlive a capture either: a replay steps the bodies behind the library's back, so a
// stepping call made during a capture ends that feature for the batch, and the question is asked for as long as it has not ended --
// also while it is switched off (dmxBatchSetLoadElision(0), DMX_ELIDE=0), since a graph recorded then is replayed all the same
// after it has been switched on.  The cost: one hipStreamIsCapturing, a host-side query, on EVERY stepping call of every batch
// that has not handed out a device pointer or been captured -- no longer only while the constants are uniform.  The exact ticks
// of small scenes, which are bound by host latency, measure what they did (configs[0] and the pen in profiles/ab_loads.txt).
inline void dmx_note_capture(dmxBatch *b)
{
    b->capturing = false;
    const bool uni = (b->elide & DMX_ELIDE_CONSTANTS) && b->uni_mass.uniform && b->uni_inertia.uniform;
    if (!uni && b->fix.ended) return;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    b->capturing = hipStreamIsCapturing(b->stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
    if (b->capturing) b->fix.end();
}
// a stepping call of the C ABI is about to advance the bodies: what dmx_state_written does, but the fixed-axis chain stands --
// the launches themselves tell the record what they are (dmx_fix_next)
inline void dmx_state_stepped(dmxBatch *b) { b->sm_mirror_valid = false; b->state_version++; b->fb_valid = false; }
// called by everything else that changes body state in the slab other than the single-launch tick
inline void dmx_state_written(dmxBatch *b) { dmx_state_stepped(b); b->fix.brk(); }

int dmx_ensure_dev(dmxBatch::DevBuf &d, size_t bytes);
// do the fused kernels make contacts (and so leave contact diagnostics behind)?  The ground plane, or static boxes on the fused path
inline bool dmx_fused_contacts(const dmxBatch *b) { return b->plane_on != 0 || (b->n_static > 0 && b->static_fast); }
// f(begin, end, thread) over contiguous chunks of [0, n) on up to DMX_HOST_THREADS (default: the host's cores, at most 16)
// threads of a persistent pool (dmx_host_pool.cpp); runs inline when n is below two grains.  The chunks must touch
// disjoint data.
namespace dmx { void host_pool_run(int nt, const std::function<void(int)> &f); }
template <class F> inline void dmx_parallel_for(int64_t n, int64_t grain, F f)
{
    static const int max_threads = [] {
        const char *e = getenv("DMX_HOST_THREADS");
        int t = e ? atoi(e) : (int)std::thread::hardware_concurrency();
        return t < 1 ? 1 : (t > 16 ? 16 : t);
    }();
    const int nt = (int)std::min<int64_t>(max_threads, n / (grain > 0 ? grain : 1));
    if (nt <= 1) { if (n > 0) f((int64_t)0, n, 0); return; }
    const int64_t per = (n + nt - 1) / nt;
    dmx::host_pool_run(nt, [&](int t) {
        const int64_t lo = t * per, hi = std::min(n, lo + per);
        if (lo < hi) f(lo, hi, t);
    });
}

struct DmxPhase {          // adds the scope's wall time to b->prof[k]
    dmxBatch *b; int k; std::chrono::steady_clock::time_point t0;
    DmxPhase(dmxBatch *bb, int kk) : b(bb), k(kk) { if (b->prof_on) t0 = std::chrono::steady_clock::now(); }
    ~DmxPhase() { if (b->prof_on) b->prof[k] += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};
// contact geometry that already lives on the device (device narrowphase): joint k's pos/normal/depth are entry src[k]
struct DevGeometry { const void *pos, *normal, *depth; const int32_t *src; };
int dmx_step_joints(dmxBatch *b, double h, int64_t n_joints, const dmxContactJoint *joints, const uint8_t *include,
                    const DevGeometry *geo, const dmxContactSurface *surfaces = nullptr);      // (surfaces: dmxBatchStepJointsSurface only)
// body-body collision handling of the batch tick (dmx_general.cpp)
int dmx_step_collide(dmxBatch *b, double h, int nsteps);
// close the chunk dmxBatchStep may have left open (flag read; rollback + replay on a violation).  Every entry point that
// observes or changes the batch calls this first.
int dmx_settle(dmxBatch *b);
// the same without breaking the fixed-axis chain (dmx_fixed.hpp): for dmxBatchStep alone, whose calls follow one another in the
// reference's loop with nothing between them; a rollback found at the close breaks the chain itself
int dmx_close_chunk(dmxBatch *b);
// the collision-checked loop in pieces (dmx_general.cpp)
int dmx_chunk_begin(dmxBatch *b, int *exact_only, int *ballistic);
int dmx_chunk_tick(dmxBatch *b, double h, int check);
int dmx_chunk_ticks(dmxBatch *b, double h, int n, int check_first, int check_last);
int dmx_check_zones(dmxBatch *b, hipStream_t st, int64_t first, int64_t count);
int dmx_chunk_end(dmxBatch *b, int *violated, int *warn);
int dmx_chunk_commit(dmxBatch *b, int ticks, int refresh_zones);
int dmx_chunk_rollback(dmxBatch *b);
int dmx_exact_tick(dmxBatch *b, double h);
int dmx_find_pairs(dmxBatch *b);           // -> b->fp_pairs / b->fp_inv
// rays_dev / ids_dev / hits_dev on the device; enqueued on the batch's stream (synchronises only to build the grid)
int dmx_ray_cast(dmxBatch *b, int64_t n_rays, const void *rays_dev, int32_t *ids_dev, void *hits_dev, uint32_t mask);


template <class T> inline void dmx_normalize_plane(const double in[4], T out[4])
{
    // dCreatePlane normalises (a,b,c,d) by |(a,b,c)| in the library's precision
    T a = (T)in[0], bb = (T)in[1], c = (T)in[2], d = (T)in[3];
    T l = a * a + bb * bb + c * c;
    if (l > 0) { l = T(1) / tsqrt<T>(l); a *= l; bb *= l; c *= l; d *= l; }
    else { a = 1; bb = 0; c = 0; d = 0; }
    out[0] = a; out[1] = bb; out[2] = c; out[3] = d;
}


template <class T> inline StepParams<T> dmx_make_params(dmxBatch *b, double h)
{
    StepParams<T> P;
    P.g = { (T)b->g[0], (T)b->g[1], (T)b->g[2] };
    P.h = (T)h;
    P.erp = (T)b->erp; P.cfm = (T)b->cfm; P.sor_w = (T)b->sor_w;
    P.iters = b->iters;
    P.gyro = b->gyro;
    P.plane_on = b->plane_on;
    T pl[4];
    dmx_normalize_plane<T>(b->plane, pl);
    P.pn = { pl[0], pl[1], pl[2] }; P.pd = pl[3];
    P.surf_mode = b->surf_mode;
    P.mu = (T)b->mu; P.bounce = (T)b->bounce; P.bounce_vel = (T)b->bounce_vel;
    P.max_contacts = b->max_contacts;
    P.elide = b->elide;
    // (not while the batch's stream is being captured into a HIP graph: dmx_note_capture)
    P.uni = (b->uni_mass.uniform && b->uni_inertia.uniform && (b->elide & DMX_ELIDE_CONSTANTS) && !b->capturing) ? 1 : 0;
    if (P.uni) {
        P.uni_mass = (T)b->uni_mass.v[0];
        P.uni_inertia = { (T)b->uni_inertia.v[0], (T)b->uni_inertia.v[1], (T)b->uni_inertia.v[2] };
    }
    { static const int nf = [] { const char *e = getenv("DMX_HULL_FILTER"); return !e ? 0 : atoi(e) == 0 ? 1 : atoi(e) == 2 ? 2 : 0; }(); P.hull_nofilter = nf; }
    P.bp_check = 0;          // set by the collision-aware tick (dmx_general.cpp)
    P.ticks = 1;
    P.bp_flags = nullptr;
    P.skip = nullptr;
    P.pack_out = (T *)b->pack_out; P.pack_lo = b->pack_lo; P.pack_hi = b->pack_hi;
    P.sbox = (const T *)b->sbox.p; P.n_static = b->n_static;
    P.sbuf = b->static_fast ? (T *)b->sbuf.p : nullptr; P.scount = (int *)b->scount.p;
    P.has_simple = b->has_simple ? 1 : 0;
    P.have8 = 1;             // (a collision-checked launch may leave the 5..8-contact launch out: fused_tick, dmx_general.cpp)
    P.hull = (const T *)b->hull.p; P.hull_n = b->hull_n;
    P.hull_planes = (const T *)b->hull_planes.p; P.hull_nf = b->hull_nf;
    P.cbuf = (T *)b->cbuf.p; P.ccount = (int *)b->ccount.p;
    return P;
}

// What is the contact-free launch of `count` bodies from slot `first` about to be enqueued with these parameters, for the
// fixed-axis words: FIX_OFF, FIX_ESTABLISH or FIX_LEAN?  Asked exactly once per launch_step call that is not handed FIX_OFF
// blindly; the record (dmx_fixed.hpp) takes the answer as given.
template <class T> inline int dmx_fix_next(dmxBatch *b, const StepParams<T> &P, int64_t first, int64_t count, bool in_place, bool ext)
{
    if (!step_is_contact_free(P)) { b->fix.brk(); return FIX_OFF; }
    FixedLaunch L;
    L.eligible = P.ticks == 1 && !ext && (P.elide & DMX_ELIDE_STORES) != 0 && !b->capturing && !b->slab_exposed && b->fix_words != nullptr;
    L.whole = first == 0 && count == b->n_active && P.skip == nullptr && P.gate == nullptr;
    L.in_place = in_place; L.bp_check = P.bp_check != 0; L.pack = P.pack_out != nullptr;
    L.key.h = FixedKey::bits(P.h);
    L.key.g[0] = FixedKey::bits(P.g.x); L.key.g[1] = FixedKey::bits(P.g.y); L.key.g[2] = FixedKey::bits(P.g.z);
    L.key.mass_uniform = (P.uni && (P.elide & DMX_ELIDE_CONSTANTS)) ? 1 : 0;
    L.key.mass = L.key.mass_uniform ? FixedKey::bits(P.uni_mass) : 0;
    L.key.gyro = P.gyro; L.key.elide = P.elide;
    L.key.n_active = b->n_active;
    return b->fix.next(L);
}
