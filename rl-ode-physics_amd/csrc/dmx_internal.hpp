// dmx_internal.hpp -- layout constants and launch interface shared by the kernels
// (dmx_kernels.hip), the batch C ABI (dmx_batch.cpp) and the ODE-compatible API (ode_compat.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dmx_math.hpp"

namespace dmx {

// Body slab layout: tiles of SLAB_TILE consecutive bodies; inside a tile the C_COUNT components are stored one
// after another, SLAB_TILE reals each (array-of-structures-of-arrays).  A wavefront stepping 64 consecutive
// bodies therefore reads and writes ONE contiguous run of memory (at most 17 x 256 B in, 13 x 256 B out in f32;
// integrate_free leaves out uniform constants and the components an in-place launch did not change)
// instead of 30 streams a whole component array apart: on MI355X that lifts the free-flight pass from
// about 5.6 to about 7.1 TB/s at 1 Mi bodies (scripts/ubench_layout.hip, profiles/r01_layout_ubench.txt).
// The slab is allocated for `stride` bodies = the body count rounded up to 256; pad bodies are valid,
// inert memory (mass 1, unit quaternion).
constexpr int SLAB_TILE = 64, SLAB_TILE_LOG2 = 6;
static_assert((1 << SLAB_TILE_LOG2) == SLAB_TILE, "tile size is a power of two");
enum : int {
    C_POS = 0,       // 3
    C_QUAT = 3,      // 4  (w,x,y,z)
    C_LVEL = 7,      // 3
    C_AVEL = 10,     // 3
    C_MASS = 13,     // 1   -- everything below is read-only during a step
    C_INERTIA = 14,  // 3
    C_SIDES = 17,    // 3
    C_FORCE = 20,    // 3   -- external accumulators, cleared by the step
    C_TORQUE = 23,   // 3
    C_BPX = 26,      // broadphase safe zone: build position x, z and radius (see dmx_broadphase.hip)
    C_BPZ = 27,
    C_BPSAFE = 28,
    C_BPR = 29,      // bounding-sphere radius (refreshed by bp_insert)
    C_COUNT = 30
};

// index of component c of body i in the slab
__host__ __device__ __forceinline__ int64_t slab_ix(int c, int64_t i)
{
    return (i >> SLAB_TILE_LOG2) * (int64_t)(C_COUNT * SLAB_TILE) + (int64_t)c * SLAB_TILE + (i & (SLAB_TILE - 1));
}

// How integrate_free's state stores leave the compute unit: a vector store with a cache-policy bit, chosen at build time.
//   STORE_PLAIN   global_store_dword[x2]
//   STORE_WT      ... sc1: written through to the fabric; the XCD's L2 drops the line (__hip_atomic_store, relaxed, agent scope)
//   STORE_NT      ... nt: non-temporal; the line stays in the XCD's L2 for the next launch's reads
// scripts/ubench_store_policy.hip measured the four forms on the lean launch's pattern (profiles/ubench_store_policy.txt): nt is
// the fastest at every shape and keeps the alternating sweep's re-reads in L2; sc1 loses them in f32.  The values are the bits
// given: no form converts.  -DDMX_STORE_POLICY=n builds the other forms for an A/B; there is no switch at run time.
enum : int { STORE_PLAIN = 0, STORE_WT = 1, STORE_NT = 2 };
#ifndef DMX_STORE_POLICY
#define DMX_STORE_POLICY 2
#endif
constexpr int kStorePolicy = DMX_STORE_POLICY;
static_assert(kStorePolicy >= STORE_PLAIN && kStorePolicy <= STORE_NT, "DMX_STORE_POLICY is 0 (plain), 1 (write-through) or 2 (non-temporal)");
#if defined(__HIPCC__)
__device__ __forceinline__ void store_state(float *p, float v)
{
    if constexpr (kStorePolicy == STORE_WT) __hip_atomic_store((uint32_t *)p, __builtin_bit_cast(uint32_t, v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else if constexpr (kStorePolicy == STORE_NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}
__device__ __forceinline__ void store_state(double *p, double v)
{
    if constexpr (kStorePolicy == STORE_WT) __hip_atomic_store((uint64_t *)p, __builtin_bit_cast(uint64_t, v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else if constexpr (kStorePolicy == STORE_NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}
#endif

// GEOM_CONVEX: the batch's one convex hull (StepParams::hull); its bounding radius sits in sides[0] like a sphere's
enum : int { GEOM_NONE = 0, GEOM_SPHERE = 1, GEOM_BOX = 2, GEOM_CONVEX = 3 };
// can a geom of class a ever produce a contact with one of class b?  Every pair of classes has a collider since round 3 (box /
// sphere / convex hull against one another: dmx_collide.hpp, dmx_collide_wave.hpp); empty slots collide with nobody, and the
// caller may switch class pairs off -- the batch's form of dGeomSetCategoryBits / dGeomSetCollideBits (main.c:724-725), which the
// reference sets per geom: bit (4 a + b) of `mask` says that classes a and b collide (dmxBatchSetClassPairs; symmetric).
constexpr uint32_t CLASS_PAIRS_ALL = 0xffffu;
__host__ __device__ __forceinline__ bool classes_collide(int a, int b, uint32_t mask)
{
    return a != GEOM_NONE && b != GEOM_NONE && ((mask >> (4 * a + b)) & 1u) != 0u;
}
constexpr int CONVEX_MAXC = 8;      // contact slots per convex body per tick (the reference's MAX_CONTACTS, main.c:675)
enum : int { SURF_BOUNCE = 0x004, SURF_SOFT_ERP = 0x008, SURF_SOFT_CFM = 0x010 };
// DMX_CONTACT_APPROX1_1 / _2: friction row 1 / 2 is bounded by mu times the contact's normal force (include/dmx_batch.h)
enum : int { SURF_APPROX1_1 = 0x1000, SURF_APPROX1_2 = 0x2000, SURF_APPROX1 = 0x3000 };
// the extended surface of dmxBatchStepJointsSurface (include/dmx_batch.h at DMX_CONTACT_MU2).  SURF_FDIR1 = DMX_CONTACT_FDIR1, the one
// bit of the seven the row builder looks at itself: what the other six select the host has resolved when it stages IslandSet::cext.
// SURF_EXT_MU1_ZERO is the host's own mark, above every bit of ODE's: mu_1 = 0 < mu_2, and cmu carries mu_2 so that the entry still
// counts three rows wherever rows are counted from cmu (contact_rpc, entry_feedback).
enum : int { SURF_FDIR1 = 0x002, SURF_EXT_MU1_ZERO = 0x10000 };
// IslandSet::cext, EXT_REALS reals per entry: mu_2 (mu_1 again without DMX_CONTACT_MU2), fdir1 as given, motion1, motion2, motionN (0
// without their bits), slip1, slip2 (-1 without their bits: the world's CFM)
enum : int { EXT_MU2 = 0, EXT_FDIR1 = 1, EXT_MOTION1 = 4, EXT_MOTION2 = 5, EXT_MOTIONN = 6, EXT_SLIP1 = 7, EXT_SLIP2 = 8, EXT_REALS = 9 };
// per-slot body flags (uint8 array)
enum : int { BF_ALIVE = 1, BF_KINEMATIC = 2, BF_NOGRAVITY = 4, BF_NOGYRO = 8 };

// Contact joints grouped by dynamics island, as the general island step consumes them.  Islands list
// their bodies (slot indices, ascending) and their contacts (creation order); body 1 of a contact is
// always a dynamic slot, body 2 is a slot or -1 (static geometry), the normal points into body 1.
template <class T> struct IslandSet {
    int n_islands;
    const int *body_off;   // [n_islands+1] into bodies
    const int *bodies;
    const int *con_off;    // [n_islands+1] into the contact arrays
    const int *row_off;    // [n_islands+1] into rows (3 rows reserved per contact)
    const T *cpos, *cnormal, *cdepth;             // 3, 3, 1 per contact
    const int *csrc;       // optional: contact c's geometry lives at index csrc[c] of gpos/gnormal/gdepth (device narrowphase output)
    const T *gpos, *gnormal, *gdepth;
    const int *cb1, *cb2, *cmode;
    const T *cmu, *cbounce, *cbounce_vel, *csoft_erp, *csoft_cfm;      // all null: every contact carries the batch's surface (StepParams)
    T *rows;               // scratch: ISLAND_ROW_REALS reals per row (29 fields), the base aligned to 256 bytes
    int *rowjb;            // scratch: 2 ints per row
    T *bscr;               // scratch: 28 reals per island body
    int *local;            // scratch: per slot, index of the body inside its island
    // large islands (solve_island_wg): per island -1 or the start of its level offsets in lev_off; per large island its
    // island index and level count; lev_rows = island-relative row indices grouped by level; crow = first row of a contact
    const int *big; int n_big; const int *big_list; const int *lev_count; const int *lev_off; const int *lev_rows;
    const int *crow;
    // launch shape of solve_island_wg: bodies of the largest such island (its accumulators go to LDS when they fit) and
    // the widest level of any schedule (64 lanes per island are enough when no level is wider)
    int big_max_bodies, big_max_width;
    int big_rows_total;    // rows of all large islands together (0: not known): bounds the schedule one of them may bring into LDS
    int big_max_rows;      // rows of the largest of them (0: not known): up to 256 x 8 (f32) a workgroup keeps them all in registers
    const int *row_level;  // level of every scheduled row, laid out like lev_rows (an island's rows start at its lev_off[0])
    const int *order;      // optional (dmxBatchSetRowOrder, DMX_ORDER_ODE): sweep `it` visits row order[(it / 8) * order_stride +
    int order_stride;      //   row_off[island] + i] at its i-th step; null: rows in creation order (solve_islands only)
    // the angular motors' prepared table (amotor_prepare, dmx_artic.hip): AMOTOR_PREP_REALS reals per joint of the set -- per axis
    // a_i and theta_i at the tick's start, in the sides as given, and the row's c, lo, hi (dmx_amotor.hpp) -- read by amotor_unit_row
    // through the index staged in the entry's cmode; null unless the tick has an AMotor row.  In IslandSet and not in StepParams for
    // the reason given below; HERE because the place decides how the island kernels' scalar registers spill: behind cext one
    // single-launch kernel gains 16 bytes of scratch, at the end of the struct another gains 32 and the solve_singles kernels change
    // registers; here no kernel gains scratch or LDS or loses a wave (profiles/amotor_kernel_resources.txt).
    const T *amotor = nullptr;
    // damping, angular speed cap, contact correction (include/dmx_batch.h, "damping").  They ride here and not in StepParams:
    // StepParams is an argument of every fused kernel too (integrate_free, step_plane, step_contacts, ...), and a field appended
    // there moves the arguments behind it in all of them.  surface_layer / max_corr_vel act on every contact's normal row; at
    // their defaults (0, +inf) the arithmetic is depth - 0 and a comparison with +inf.  damping: the per-slot table on the device,
    // DAMP_REALS reals per slot (dmx_damping.hpp), null unless some slot's maximum angular speed is finite: finish_body then loads
    // nothing.  (Where the three stand among the fields decides how small_world_tick's scalar registers spill: here no kernel's
    // scratch grows over the parent's, at the end of the struct three instantiations' did -- profiles/stability_kernel_resources.txt.)
    T surface_layer = T(0), max_corr_vel = (T)__builtin_huge_val();
    const T *damping = nullptr;
    // an extended tick (dmxBatchStepJointsSurface with some bit of DMX_CONTACT_SURFACE_EXT honoured): EXT_REALS reals per entry behind
    // the contact arrays' twelve, read by contact_rows' APX instantiations only; null in every other tick.  (Here, behind the damping
    // table, and not at the end of the struct, for the reason given above: at the end small_world_tick<float, true, false, false, true>
    // gains 32 bytes of scratch and the two solve_singles kernels change registers; here every kernel that is not an APX
    // instantiation keeps the parent's registers, scratch, occupancy and LDS -- profiles/surface_kernel_resources.txt.)
    const T *cext = nullptr;
    int singles;           // 1: islands of one body with 1..8 contacts are left to solve_singles / solve_singles_lds (one lane each);
                           // whoever builds `big` must then keep such islands out of it
    // 1: some entries of the contact arrays are units of articulation joints (dmx_island_rows.hpp: joint_unit_rows), marked by
    // cmu = UNIT_*_MU; within an island they come before its contacts.  0: contacts only
    int has_units = 0;
};
// dmxBatchSetFeedback: what a tick made with feedback on carries beside its IslandSet.  Such a tick launches the island kernels'
// FB instantiations (launch_islands, launch_small_tick), which are kernels of their own: a tick without feedback runs the code
// it would run if feedback did not exist, and takes no FeedbackSet's worth of arguments it never reads into account.
// mode: FB_UNSCALED: the rows' J is as built (dWorldStep's solves); FB_SCALED: row_setup<T, true, true> multiplied it by Ad and
// left Ad in the row's slot RW_UNSCALE.  Per entry of the contact arrays: out = the result's index (a joint of the set: its
// index; a contact joint: the set's size + its index in the caller's list) when the entry is the first of its joint, else -1;
// info = 2 x (entries of the joint, which are adjacent) + (1: the sides were exchanged); isl = the entry's island (read by the
// general path's kernel only).  fb: 12 reals per result (f1, t1, f2, t2 in the sides as given), zeroed before the tick.
enum : int { FB_OFF = 0, FB_UNSCALED = 1, FB_SCALED = 2 };
template <class T> struct FeedbackSet {
    int mode = FB_OFF;
    const int *out = nullptr, *info = nullptr, *isl = nullptr;
    T *fb = nullptr;
};
// a unit's marker in IslandSet::cmu: a negative number (for the first three minus the row count; a contact's mu is never negative there when has_units is set)
// (UNIT_LIMOT: a hinge's limit / motor row, dmxBatchSetHingeLimots -- the one unit whose row can clamp)
// (UNIT_LOCK: the three angular rows of a slider or a fixed joint; UNIT_SLIDER2: a slider's two linear rows; UNIT_SLIMOT: a slider's
//  limit / motor row, which can clamp as a hinge's can.  Their markers are distinct numbers below the others: a unit's row count
//  comes from its kind, unit_rows_of in dmx_island_rows.hpp and rpc_of in dmx_joints.cpp)
// (UNIT_AMOTOR: one axis of an angular motor, dmxBatchSetAMotors -- one row that can clamp, below UNIT_SLIMOT_MU)
constexpr int UNIT_BALL = 1, UNIT_HINGE2 = 2, UNIT_LIMOT = 3, UNIT_LOCK = 4, UNIT_SLIDER2 = 5, UNIT_SLIMOT = 6, UNIT_AMOTOR = 7;
constexpr double UNIT_BALL_MU = -3.0, UNIT_HINGE2_MU = -2.0, UNIT_LIMOT_MU = -1.0, UNIT_LOCK_MU = -4.0, UNIT_SLIDER2_MU = -5.0, UNIT_SLIMOT_MU = -6.0,
                 UNIT_AMOTOR_MU = -7.0;
// the angular motors' prepared table (IslandSet::amotor; written by amotor_prepare_joint, dmx_amotor.hpp, read by amotor_unit_row,
// dmx_island_rows.hpp): per joint of the set, per axis i = 0, 1, 2, eight reals -- a_i (3), theta_i, then c, lo, hi of the axis's row
// by the five-line table, and a spare -- axis i of joint j stands at AMOTOR_PREP_REALS j + AMOTOR_AXIS_REALS i
enum : int { AMOTOR_AXIS_REALS = 8, AMOTOR_PREP_REALS = 3 * AMOTOR_AXIS_REALS };
enum : int { AMP_AXIS = 0, AMP_THETA = 3, AMP_C = 4, AMP_LO = 5, AMP_HI = 6 };
// Is a hinge's limot row there?  fmax > 0, or a finite stop.  Decided on the parameters alone -- the host sizes islands, schedules and LCP
// scratch before the device has looked at the angle, so the row count must not depend on the state -- and in this one place: the
// batch's tick (dmx_joints.cpp) and the ODE face (ode_compat.cpp: whether to hand the batch limots at all) must agree.
inline bool limot_present(double lo_stop, double hi_stop, double fmax)
{
    const double inf = __builtin_huge_val();
    return fmax > 0 || (lo_stop > -inf && lo_stop < inf) || (hi_stop > -inf && hi_stop < inf);
}

template <class T> struct StepParams {
    V3<T> g;            // gravity
    T h;                // step size
    T erp, cfm, sor_w;  // world ERP, CFM, SOR over-relaxation
    int iters;          // QuickStep iterations
    int gyro;           // 0 off, 1 explicit, 2 implicit
    int plane_on;       // ground half-space present
    V3<T> pn; T pd;     // plane n.x = d
    int surf_mode; T mu, bounce, bounce_vel;   // contact surface (NearCallback, main.c:684-687)
    int max_contacts;
    int hull_nofilter;  // DMX_HULL_FILTER=0: the hull colliders' conservative filter lets every point through (A/B, diagnosis)
    int bp_check;       // safe-zone test of every body's pre-step position (BPC_* bits; any bit = "this tick" for one-tick kernels)
    int ticks;          // integrate_free: ticks taken by one launch with the state held in registers (>= 1)
    uint32_t *bp_flags; // device flags (BPF_*), written when a body has left its safe zone
    const uint8_t *skip; // per-body: 1 = stepped by the island path this tick, leave untouched (may be null)
    // boundary-row pack for the multi-GPU exchange (null = off): bodies i < pack_lo and i >= pack_hi also write
    // their new 13-real state to pack_out[slot*13 ..], slot = i (lower row) or pack_lo + i - pack_hi (upper row)
    T *pack_out; int64_t pack_lo, pack_hi;
    // convex bodies: the shared hull (hull_n body-frame points, 3 reals each) and the tick's ground-plane contacts of
    // every convex body, written by np_convex_plane and read by step_plane: cbuf[i][k] = (x, y, z, depth), ccount[i]
    const T *hull; int hull_n;
    const T *hull_planes; int hull_nf;      // the hull's faces: unit outward normal + offset, body frame (box-convex collider)
    T *cbuf; int *ccount;
    // static (body-less) box geoms, AddBodyMap main.c:735-761: SBOX_REALS reals each (see SBOX_*); the safe-zone test of the
    // fused kernels also asks that a body's bounding sphere stays clear of every static box's AABB
    const T *sbox; int n_static;
    // the fused path of bodies at static boxes (np_static / np_convex_static -> step_contacts, dmx_kernels.hip): every body's
    // contacts with the ground plane and the static boxes, creation order, canonical form (normal into the body), in tiles
    // like the slab's (sc_ix); scount[i] = their number, SC_MAXC + 1 = more than the buffer holds.  have8: the launch
    // for bodies with 5..8 contacts follows the one for 0..4 (otherwise the latter reports BPF_NEED8 when it meets one)
    T *sbuf; int *scount; int have8;
    int has_simple;     // the batch has box / sphere bodies (0: np_static, which serves those, need not be launched)
    // a launch enqueued before the host knows whether it should run (careful_tick's speculative tick): the fused kernels
    // return at once unless *gate != 0 (ExactCounts::spec_ok on the device).  Null: no question asked.
    const uint32_t *gate = nullptr;
    // integrate_free, work the result does not need (dmxBatchSetElision): bit 0 = an in-place launch stores only the components
    // some body of the wavefront changed; bit 1 = when every slot has the same mass and inertia (uni = 1; dmx_uniform.hpp
    // keeps track) they travel as arguments, uni_mass / uni_inertia, and the kernel does not load them
    int elide = 0, uni = 0;
    T uni_mass = T(1); V3<T> uni_inertia = { T(1), T(1), T(1) };
};
// contact buffer of the static fused path: SC_MAXC contacts of SC_REALS reals per body, field f of contact k of body i at
// sbuf[sc_ix(k, f, i)] -- tiles of 64 bodies, so a wavefront's access to one field of one contact is one contiguous run
constexpr int SC_MAXC = 8;
enum : int { SC_POS = 0, SC_NORMAL = 3, SC_DEPTH = 6, SC_REALS = 7 };
__host__ __device__ __forceinline__ int64_t sc_ix(int k, int f, int64_t i)
{
    return ((i >> SLAB_TILE_LOG2) * (int64_t)(SC_MAXC * SC_REALS) + (int64_t)(k * SC_REALS + f)) * SLAB_TILE + (i & (SLAB_TILE - 1));
}
// reals per constraint row in the island kernels' row scratch (IslandSet::rows): 29 fields, padded to one aligned line
constexpr int ISLAND_ROW_REALS = 32;
// islands of up to this many rows: one wavefront of solve_island_wg, rows in registers, only row_level of the schedule read
constexpr int WAVE_ISLAND_ROWS = 256;
// layout of one static box in StepParams::sbox / GridParams::sbox
enum : int { SBOX_POS = 0, SBOX_R = 3, SBOX_SIDE = 12, SBOX_LO = 15, SBOX_HI = 18, SBOX_REALS = 24 };
constexpr int MAX_STATIC_BOXES = 64;

// StepParams::bp_check for a launch of `ticks` ticks: test at every tick, or only at the launch's first / last tick
enum : int { BPC_ALL = 1, BPC_FIRST = 2, BPC_LAST = 4 };
// hashed (x,z)-column grid of the body-body broadphase
// (BPF_VIOLATION .. BPF_NEED8 are the chunk's flags, cleared together when a chunk begins.  BPF_NOFAST: a body has more contacts
// with static geometry than the fused path's buffer holds -- only the exact path can step it; BPF_NEED8: a body has 5..8 and
// the launch for those was not enqueued.  Both come with BPF_VIOLATION.)
enum : int { BPF_OVERFLOW = 0, BPF_CROWDED = 1, BPF_NPAIRS = 2, BPF_VIOLATION = 3, BPF_WARN = 4, BPF_NOFAST = 5, BPF_NEED8 = 6, BPF_COUNT = 7 };
constexpr int BPF_CHUNK_FLAGS = 4;      // VIOLATION, WARN, NOFAST, NEED8
// per body, left by grid_insert for the exact pair search: its column and its AABB in one aligned record (32 B f32, 64 B f64),
// so a candidate costs one access, not eight
template <class T> struct alignas(16) GridRec { T lo[3], hi[3]; int32_t ix, iz; };
template <class T> struct GridParams {
    T cell, inv_cell, r_max;
    T r_cls[4];            // largest bounding radius per geometry class (0: the batch has none of it): what a body of a class can
                           // meet outside its 3x3 block of columns is bounded by the classes it collides with (classes_collide)
    uint32_t mask;         // table size - 1 (power of two)
    int xbits;             // > 0: the table is a 2-D torus of 2^xbits columns per row (neighbouring cells are neighbouring
                           // entries: coalesced lookups); 0: scrambled hash (scenes too elongated for the torus)
    int cap;               // bodies per bucket
    uint32_t *count;       // [mask+1]
    int32_t *items;        // [(mask+1) * cap]
    uint32_t *flags;       // [BPF_COUNT]
    GridRec<T> *rec;       // optional [per slot]: bp_insert leaves every body's column and AABB here for the exact pair search
    const T *sbox; int n_static;   // static boxes (StepParams::sbox)
    // 1: bodies at static boxes take the fused path (step_contacts) unless their contacts might not fit its buffer -- AABB
    // over two or more static boxes, or over one with a ground plane present: only those are "involved" in an exact tick,
    // and being near a static box does not make a body crowded.  0 (DMX_STATIC_FAST=0): every body at a static box is.
    int static_fast, plane_on;
    const T *hull; int hull_n;     // the batch's hull shape (convex bodies' exact AABBs for the pair search: bp_convex_aabb)
    uint32_t class_pairs;          // which geometry classes collide with which (classes_collide)
};

// ray casts (dmx_raycast.hip).  Result ids below zero, the visibility mask's bits (bit gt - 1 for a body of class gt) and the forms
// are the values of include/dmx_batch.h (DMX_RAY_*); dmx_general.cpp holds the static_asserts.
enum : int { DMX_RAYID_MISS = -1, DMX_RAYID_PLANE = -2 };       // static box k: -3 - k
enum : uint32_t { DMX_RAYMASK_BODIES = 7u, DMX_RAYMASK_STATIC = 8u, DMX_RAYMASK_PLANE = 16u };
enum : int { RAY_FORM_AUTO = 0, RAY_FORM_LANE = 1, RAY_FORM_WAVE = 2, RAY_FORM_BRUTE = 3 };
template <class T> struct RaySceneParams {
    const T *S; const uint8_t *gtype; const uint8_t *bflags; int64_t n;     // every slot of [0, n) can be seen, ghost slots too
    const T *hull_planes; int hull_nf;
    const T *sbox; int n_static;
    int plane_on; V3<T> pn; T pd;
    uint32_t mask;
    // the ray cast's own column grid (same hashing and bucket layout as GridParams) and the visible bodies' (x,z) rectangle
    // (xmin, xmax, zmin, zmax as ordered keys: dmx_raycast.hip)
    T cell, inv_cell;
    uint32_t gmask; int xbits, cap;
    const uint32_t *count; const int32_t *items;
    const unsigned long long *rect;
};

struct StepDiag {
    unsigned long long contacts;
    double residual;
};

// S: the slab the tick reads (state, constants, zones); So: the slab the new state is written to -- S itself for an
// in-place tick, or the batch's other slab (constants and zones are kept identical in both), which leaves S's state
// behind untouched: the zero-cost snapshot of a collision-proof chunk (dmx_general.cpp).
// rev: the direction in which a contact-free launch (integrate_free) walks the tiles (dmx_sweep.hpp; dmx_next_sweep in
// dmx_batch_priv.hpp hands out alternating ones); the kernels of ticks with contacts take no notice of it.
// fix_mode / fix_words: what dmx_fixed.hpp's record said about a contact-free launch (FIX_OFF = 0: the launch it always was),
// and the batch's word per tile; a launch that does not reach integrate_free must come with FIX_OFF.
// torque_free: the batch's switch for the short tick of a body without torque (dmx_torque_free.hpp decides per launch whether it
// applies); off, the launch is the one it always was.  tf_stats: two counters of the caller's, [0] contact-free launches that took an
// instantiation with the short tick, [1] those that did not (dmxBatchTorqueFreeStats).
// lean_kernel: the batch's switch for integrate_free_lean, the straight-line kernel of a lean launch (dmx_kernels.hip: launch_step
// has the rule); off, the launch is the one it always was.  lk_stats: two counters of the caller's, [0] contact-free launches that
// took that kernel, [1] those that did not (dmxBatchLeanKernelStats).
template <class T>
hipError_t launch_step(T *S, T *So, const uint8_t *gtype, int64_t stride, int64_t n, const StepParams<T> &P, bool ext,
                       StepDiag *diag, hipStream_t st, int rev, int fix_mode = 0, uint32_t *fix_words = nullptr, bool torque_free = false,
                       int64_t *tf_stats = nullptr, bool lean_kernel = false, int64_t *lk_stats = nullptr);
// does launch_step take these parameters to integrate_free (no plane, no static geometry with contact slots)?
template <class T> inline bool step_is_contact_free(const StepParams<T> &P)
{
    return !(P.n_static > 0 && P.sbuf != nullptr) && !P.plane_on;
}
template <class T>
hipError_t launch_islands(T *S, const uint8_t *bflags, int64_t stride, const IslandSet<T> &I, const StepParams<T> &P,
                          StepDiag *diag, hipStream_t st, bool feedback = false, bool pyramid = false);      // (feedback, pyramid: the kernels' FB / APX instantiations)
// feedback of a dmxBatchStepJoints tick on the general path (dmx_artic.hip): one lane per entry, behind the tick's solves
template <class T>
hipError_t launch_feedback(const IslandSet<T> &I, const StepParams<T> &P, const FeedbackSet<T> &F, int n_entries, hipStream_t st);
// dWorldStep: solve_islands for the islands without rows only (those with rows: launch_lcp_lds / lcp_grid_solve, dmx_lcp.hpp)
template <class T>
hipError_t launch_islands_without_rows(T *S, const uint8_t *bflags, int64_t stride, const IslandSet<T> &I, const StepParams<T> &P,
                                       StepDiag *diag, hipStream_t st);
// bucket counts and flags to zero, and two optional small records (each at most 256 words) with them
hipError_t launch_bp_clear(uint32_t *count, size_t n_count, uint32_t *flags, void *rec_a, size_t bytes_a, void *rec_b, size_t bytes_b,
                           hipStream_t st);
template <class T>
hipError_t launch_bp_insert(T *S, const uint8_t *gtype, int64_t stride, int64_t n, const GridParams<T> &G, hipStream_t st);
// the exact world AABB of every convex body among [0, n) into G.rec (one wavefront per hull), over the bounding sphere's box
// bp_insert left there
template <class T>
hipError_t launch_bp_convex_aabb(const T *S, const uint8_t *gtype, int64_t n, const GridParams<T> &G, hipStream_t st);
template <class T>
hipError_t launch_bp_safe_zone(T *S, const uint8_t *gtype, int64_t stride, int64_t n_active, const GridParams<T> &G, hipStream_t st);
// ground-plane contacts of the convex bodies among [0, n): one wavefront per body walks the hull (dCollideConvexPlane)
template <class T>
hipError_t launch_np_convex_plane(const T *S, const uint8_t *gtype, int64_t n, const StepParams<T> &P, hipStream_t st);
// contacts of bodies [0, n) with the ground plane and the static boxes -> P.sbuf / P.scount (boxes and spheres one lane each,
// convex hulls one wavefront each); bodies masked by P.skip are left alone
template <class T>
hipError_t launch_np_static(const T *S, const uint8_t *gtype, int64_t n, const StepParams<T> &P, hipStream_t st);
template <class T>
hipError_t launch_pack_transforms(const T *S, int64_t stride, int64_t first, int64_t count, T *out, hipStream_t st);
template <class T>
hipError_t launch_gather(const T *S, int64_t stride, const int32_t *idx, int64_t count, T *out, hipStream_t st);
template <class T>
hipError_t launch_scatter(T *S, int64_t stride, const int32_t *idx, int64_t count, const T *in, hipStream_t st);
// safe-zone test of slots [first, first+count) only (no integration): raises BPF_VIOLATION / BPF_WARN in `flags`
template <class T>
hipError_t launch_check_zones(const T *S, int64_t first, int64_t count, uint32_t *flags, hipStream_t st);
// ghost slots [first, first+count_lo) <- src_lo, the next count_hi <- src_hi (13-real AoS rows; null = leave alone), with
// an optional safe-zone test of the new positions
template <class T>
hipError_t launch_refresh_ghosts(T *S, int64_t first, int64_t count_lo, const T *src_lo, int64_t count_hi, const T *src_hi,
                                 int check, uint32_t *flags, hipStream_t st);
template <class T>
hipError_t launch_fill_component(T *S, int c, T value, int64_t n, hipStream_t st);
// rollback snapshot of the 13 state components of bodies [0, n_bodies): save = slab -> packed, else packed -> slab
template <class T>
hipError_t launch_copy_state(T *S, T *packed, int64_t n_bodies, bool save, hipStream_t st);
// components [c0, c0+k) of bodies [first, first+count) from one slab to the other (same layout)
template <class T>
hipError_t launch_copy_components(const T *from, T *to, int c0, int k, int64_t first, int64_t count, hipStream_t st);
template <class T>
hipError_t launch_aos_to_soa(T *S, int64_t stride, int comp0, int k, int64_t first, int64_t count, const T *aos,
                             hipStream_t st);
template <class T>
hipError_t launch_soa_to_aos(const T *S, int64_t stride, int comp0, int k, int64_t first, int64_t count, T *aos,
                             hipStream_t st);

// the (x,z) bounding rectangle of the centres of the slots a ray can see (class set, alive) -> rect[4]
template <class T>
hipError_t launch_ray_bounds(const T *S, const uint8_t *gtype, const uint8_t *bflags, int64_t n, unsigned long long *rect, hipStream_t st);
// n_rays rays (7 reals each: origin, direction, length) -> ids, hits (7 reals each: pos, normal, depth); form = RAY_FORM_LANE / WAVE / BRUTE
template <class T>
hipError_t launch_ray_cast(int form, const RaySceneParams<T> &Sc, int64_t n_rays, const T *rays, int32_t *ids, T *hits, hipStream_t st);
hipError_t dmx_touch_raycast(int real_bytes);

// one per translation unit with device code: forces the unit's code object to load (see dmx_kernels.hip)
hipError_t dmx_touch_kernels(int real_bytes); hipError_t dmx_touch_islands(int real_bytes); hipError_t dmx_touch_broadphase(int real_bytes);
hipError_t dmx_touch_narrow(int real_bytes); hipError_t dmx_touch_exact(int real_bytes);

}  // namespace dmx
