// dmx_kernels.hip -- gfx950 kernels of the rigid-body step hot path.
//
// Replaces, per tick, the three ODE calls of the reference's physics loop
// (/root/reference/src/main.c:211-215): dSpaceCollide + NearCallback
// (main.c:674-693), dWorldStep stepped with QuickStep semantics, and
// dJointGroupEmpty -- for scenes whose dynamics islands are single bodies
// (free bodies, and bodies in contact with the static ground plane only).
//
// Data layout: one slab `S` of `real` in tiles of 64 bodies x 30 components
// (dmx_internal.hpp: component c of body i at S[slab_ix(c, i)]), so that a
// wavefront's 30 component accesses fall in one contiguous 7.5 KiB (f32) run.
// A lane owns one body.
//
// No MFMA: there is no dense contraction on this path.  integrate_free is
// HBM-bound (at most 30 reals per body-step, 19 on a dropped unit-mass scene:
// see the kernel's header); step_plane is VALU/latency bound (20 SOR sweeps
// over <= 12 rows held in registers).
#include <hip/hip_runtime.h>
#include <type_traits>
#include "dmx_internal.hpp"
#include "dmx_math.hpp"
#include "dmx_collide.hpp"
#include "dmx_step_fused.hpp"
#include "dmx_sweep.hpp"
#include "dmx_fixed.hpp"
#include "dmx_torque_free.hpp"
#include "dmx_launch_consts.hpp"
#include "dmx_lean_tick.hpp"

namespace dmx {

// ---------------------------------------------------------------------------------------------
// integrate_free: contact-free tick (BASELINE config 2/4).  Algorithmic traffic per body-step, at most:
// read 13 state + 4 constant reals, write 13 state reals = 30 reals (120 B f32 / 240 B f64).
// OPT (StepParams::elide, dmxBatchSetElision) takes out what the result does not need:
//   OPT_ELIDE  an IN-PLACE launch (So == S) stores component k of a wavefront's 64 bodies only if some lane's new
//              value differs in its BITS from the one loaded (-0.0 -> +0.0 and NaN payloads count as changes): the
//              store would have put back what is there.  One ballot and one scalar branch per component; a run that
//              is stored is stored whole, for all 64 lanes.  An out-of-place launch (the first of a collision-proof
//              chunk) stores all 13, as OPT = 0 does.
//   OPT_UNI    mass and inertia are the same for every slot (dmx_uniform.hpp keeps track, host side): they arrive
//              as kernel arguments (StepParams::uni_mass / uni_inertia) and components 13..16 are not loaded.  What the tick
//              computes from them and h alone -- 1 / Ib.k, 1 / h, the isotropy test; h * (1 / m) and m g -- comes with them, computed
//              once on the host with the tick's own operations (`lc`, dmx_launch_consts.hpp; `tf`): left in the kernel, the compiler
//              hoists it ahead of the loop, 75 vector instructions with five IEEE divisions in front of every wavefront's first
//              load.  A launch whose constants the rule of dmx_launch_consts.hpp refuses (zero, inf, NaN) is one without OPT_UNI.
// A dropped scene of unit-mass bodies under gravity along y (the reference's AddBody + dWorldSetGravity) then moves
// 13 reals in and 6 out (pos.y, quat, lvel.y) = 19 per body-step; any other scene moves what it changes, up to the 30.
// Same values into the same free_body_step either way: same bits.
//   FIX        (a template parameter of its own, not a bit of OPT: dmxBatchSetElision keeps its two) the one-tick kernels with
//              store elision also exist with the fixed-axis mode built in, for launches over the whole active slab that
//              dmx_fixed.hpp's record has called establishing or lean (fix_mode, a scalar argument of its own like `rev`).  A word
//              per 64-body tile (fix_words) says in bits 0..2 that a launch loaded pos.k and lvel.k of the tile's active lanes, ran
//              the tick and found both unchanged in every lane's bits -- the very ballots of the store elision.  The tick computes
//              them from themselves, h, g.k and the mass alone, so they stay for as long as the record's chain is unbroken.  An
//              establishing launch loads all 13 and writes every tile's word; a lean one reads the word, issues neither the two
//              loads nor the ballots and stores of a fixed lateral axis (x, z), tests a clear axis as an establishing launch does
//              and rewrites a word that changes (-0.0 -> +0.0 clears the bit in the tick where it happens).  The dropped scene
//              then moves 9 reals in and 6 out = 15 per body-step.  Every other launch is the kernel without FIX, as it always was.
//   TF         Short tick (dmx_torque_free.hpp has the rule, dmx_step_fused.hpp: free_body_step_torque_free the code): with OPT_UNI and
//              without EXT the launch's torque can be known to be exactly (+0, +0, +0) -- no accumulators, no gyroscopic torque -- and
//              then the general tick's w += Iw^-1 (h tacc) is w + (+0) for every finite Iw^-1.  `tf` (scalar arguments of their own,
//              StepParams does not grow) says whether that holds for this launch and carries hm = h * (1 / m) and mg = m g, computed
//              once on the host with the tick's own operations.  A launch for which it holds takes the instantiation with TF: a
//              wavefront whose every active lane has |q.k| <= 2 (one ballot, one scalar branch; per tick in the many-ticks kernel)
//              builds neither R nor R diag(1/Ib) R^T -- a quarter of the vector instructions the headline's tick executes; any other
//              wavefront runs tick_head and tick_tail in the same kernel.  A template parameter and not a branch on tf.on alone: the
//              general tick behind the join costs 18 more vector instructions than free_body_step, which a launch that can never
//              take the short way measured as 0.3 us per tick at 1 Mi bodies (profiles/ab_torque_free_first_build.txt); every launch with
//              tf.on = 0 is the kernel without TF, as it always was.  Same bits (tests/test_torque_free.py on the host over
//              1 Mi bodies per precision, tests/test_gpu_torque_free.py on the device); registers as before
//              (profiles/torque_free_resources.txt).
// Sweep order (dmx_sweep.hpp): `rev` -- a scalar argument of its own, StepParams does not grow -- says in which direction this
// launch walks the tiles; workgroup b works on tile group sweep_block(b, gridDim.x, rev).  The callers alternate it from one
// contact-free launch to the next, so that the lines the last launch touched last, still in the XCDs' L2s, are read first.  The
// grid is a multiple of 8 workgroups (launch_step rounds it up; the surplus ones find their bodies at or beyond n and leave),
// which keeps a tile group on the same residue b % 8, hence -- as the dispatcher is observed to deal -- on the same XCD, in both
// directions.  Which workgroup steps a body changes nothing in the body's tick: same bits in either direction.
// ---------------------------------------------------------------------------------------------
enum : int { OPT_ELIDE = 1, OPT_UNI = 2 };
template <class T> struct BitsOf;
template <> struct BitsOf<float> { using type = uint32_t; };
template <> struct BitsOf<double> { using type = uint64_t; };
template <class T> __device__ __forceinline__ bool bits_differ(T a, T b)
{
    using U = typename BitsOf<T>::type;
    return __builtin_bit_cast(U, a) != __builtin_bit_cast(U, b);
}

// the tile's axis (x, y, z = 0, 1, 2) a state component belongs to for the fixed-axis words: pos and lvel; -1 for quat and avel
__host__ __device__ constexpr int fix_axis_of(int k) { return k < C_QUAT ? k - C_POS : (k >= C_LVEL && k < C_AVEL) ? k - C_LVEL : -1; }

template <class T, bool EXT, int MINW, bool MULTI, int OPT = 0, bool FIX = false, bool TF = false>
__global__ __launch_bounds__(256, MINW) void integrate_free(T *S, T *So, int64_t n, StepParams<T> P, int rev, int fix_mode,
                                                            uint32_t *fix_words, TorqueFree<T> tf, LaunchConsts<T> lc)
{
    constexpr bool ELIDE = (OPT & OPT_ELIDE) != 0, UNI = (OPT & OPT_UNI) != 0;
    static_assert(!FIX || (ELIDE && !EXT && !MULTI), "the fixed-axis mode is built into the one-tick kernels with store elision only");
    static_assert(!TF || (UNI && !EXT), "the short tick needs the constants as arguments and no force accumulators");
    constexpr int NLOAD = UNI ? C_MASS : C_SIDES;      // components read: the state, and the constants unless they are arguments
    // So = where the new state goes: S itself (in place) or the batch's other slab (the first launch of a
    // collision-proof chunk, which thereby leaves the chunk's start state behind as the rollback snapshot)
    // (FIX: launch_step refuses such a launch with a gate or a skip mask, and the kernel relies on it -- it reads neither pointer,
    //  which spares the wavefront a scalar load and its wait ahead of everything else)
    if constexpr (!FIX) {
        if (P.gate != nullptr && *P.gate == 0u) return;
    }
    const int nticks = MULTI ? P.ticks : 1;         // MULTI = false: the one-tick kernel, no loop
    const bool in_place = ELIDE && So == S;         // wave-uniform: two kernel arguments
    for (int64_t i = sweep_block(blockIdx.x, gridDim.x, rev) * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
#include "dmx_free_tile.inc"
    }
}

// ---------------------------------------------------------------------------------------------
// integrate_free_lean: the lean launch (FIX_LEAN) of integrate_free<T, false, MWU, false, 3, true, true> as a kernel of its own,
// for launches the host already knows to be lean, in place, one tick, with the constants as arguments and the short tick on
// (launch_step has the rule).  What such a launch's wavefront needs stands in LeanHot (dmx_lean_tick.hpp) at the head of the
// arguments; the kernel asks for nothing else ahead of its loads -- neither StepParams nor the dispatch packet -- has no grid-stride
// loop (one tile per wavefront: launch_step's grid covers every tile) and tests nothing the host has decided.
//   Straight line: a wavefront whose word has both lateral bits set and whose active lanes all pass torque_free_admits.  The word's
//   load first, the nine loads behind it, lean_tick, nine ballots with the elided stores, and the word rewritten if its y bit changes.
//   Any other wavefront -- a clear lateral axis, a lane that fails the guard -- runs dmx_free_tile.inc, the very body of the
//   kernel this one stands in for, from its own loads on: nothing has been stored by then.
// Same bits either way (tests/test_lean_tick.py on the host, tests/test_gpu_lean_kernel.py on the device).  64-bit indexing as
// everywhere.  No launch bound beyond the workgroup's size (profiles/lean_kernel_resources.txt has the candidate with one).
// ---------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void integrate_free_lean(LeanHot<T> A, StepParams<T> P, TorqueFree<T> tf, LaunchConsts<T> lc)
{
    const int64_t i = sweep_block(blockIdx.x, A.g8, A.rev) * (int64_t)256 + threadIdx.x;
    if (i >= A.n) return;
    T *t = A.S + slab_ix(0, i);         // component k of body i is t[k * SLAB_TILE]
    const uint32_t word = A.fix_words[__builtin_amdgcn_readfirstlane((int)(i >> 6))];
    // pos.y, quat, lvel.y, avel
    constexpr int NK = 9;
    constexpr int comp[NK] = { C_POS + 1, C_QUAT, C_QUAT + 1, C_QUAT + 2, C_QUAT + 3, C_LVEL + 1, C_AVEL, C_AVEL + 1, C_AVEL + 2 };
    T was[NK];
#pragma unroll
    for (int k = 0; k < NK; k++) was[k] = t[comp[k] * SLAB_TILE];
    const uint32_t seen = __builtin_amdgcn_readfirstlane(word);
    Q4<T> q = { was[1], was[2], was[3], was[4] };
    if ((seen & 5u) != 5u || __ballot(!torque_free_admits(q)) != 0ull) {
        // the tile as integrate_free<T, false, MWU, false, 3, true, true> steps it in a lean launch in place: the fragment's names
        constexpr bool EXT = false, FIX = true, TF = true, ELIDE = true, UNI = true, in_place = true;
        constexpr int NLOAD = C_MASS, fix_mode = FIX_LEAN, nticks = 1;
        T *const S = A.S, *const So = A.S;
        uint32_t *const fix_words = A.fix_words;
        do {        // (a `continue` of the fragment leaves the tile)
#include "dmx_free_tile.inc"
        } while (false);
        return;
    }
    T xy = was[0], vy = was[5];
    V3<T> w = { was[6], was[7], was[8] };
    lean_tick(xy, q, vy, w, A.hm, A.mgy, A.h);
    const T now[NK] = { xy, q.w, q.x, q.y, q.z, vy, w.x, w.y, w.z };
    uint32_t moved = 0;             // bit 1: some lane's pos.y or lvel.y changed its bits in this tick
#pragma unroll
    for (int k = 0; k < NK; k++) {
        const bool changed = __ballot(bits_differ(now[k], was[k])) != 0ull;
        if (fix_axis_of(comp[k]) == 1 && changed) moved |= 2u;
        if (!changed) continue;
        store_state(&t[comp[k] * SLAB_TILE], now[k]);
    }
    // (the lateral axes were not loaded and keep their bits: same inputs, same bits)
    const uint32_t neww = ~moved & 7u;
    if (neww != seen && (threadIdx.x & 63) == 0) A.fix_words[i >> 6] = neww;
}

// ---------------------------------------------------------------------------------------------
// step_plane: fused tick for single-body islands resting on / falling onto the ground plane
// (BASELINE config 1/3): narrowphase -> contact rows (normal + 2 friction per contact) ->
// SOR-PGS sweeps -> velocity update -> integrate.  One lane per body; rows live in registers.
// Algorithmic traffic per body-step: 13 + 4 + 3 (sides) read, 13 written = 33 reals.
// ---------------------------------------------------------------------------------------------
// NC = contact slots per body: 4 (box-plane yields at most 4 contacts) or CONVEX_MAXC when the batch has convex bodies,
// whose plane contacts np_convex_plane left in P.cbuf.
template <class T, bool EXT, int MINW, int NC>
__global__ __launch_bounds__(256, MINW) void step_plane(T *S, T *So, const uint8_t *__restrict__ gtype,
                                                  int64_t stride, int64_t n, StepParams<T> P,
                                                  StepDiag *__restrict__ diag)
{
    step_plane_body<T, EXT, NC>(S, So, gtype, stride, n, P, diag, blockIdx.x * (int64_t)blockDim.x + threadIdx.x);
}

// ---------------------------------------------------------------------------------------------
// step_contacts: fused tick for single-body islands at STATIC GEOMETRY -- the ground plane and the static boxes
// (AddBodyMap, main.c:735-761; the reference's floor is one, main.c:115).  The contacts come from np_static /
// np_convex_static (dmx_narrow.hip) in joint creation order and canonical form; here: rows (normal + 2 friction per
// contact, every contact with its own normal) -> SOR-PGS sweeps -> velocity update -> integrate, one lane per body, rows in
// registers.  Around the rows the tick is tick_head / tick_tail (dmx_step_fused.hpp), as in step_plane_body and free_body_step; the
// loads, rows, sweep, stores and diagnostics are a second copy of step_plane_body's, with every contact's own normal and M^-1 J^T's
// linear part kept per row: change both -- the measured reason stands there (same bits as the oracle, tests/test_gpu_static.py).
// Two instantiations share a tick: NC = 4 steps the bodies with 0..4 contacts (free bodies included), NC = 8 -- launched
// behind it when the batch may have such bodies (P.have8) -- those with 5..8; each leaves the other's lanes alone.  A body
// with more contacts than the buffer holds raises BPF_NOFAST (the exact path steps it: the chunk is rolled back).
// Algorithmic traffic per body-step: 13 + 4 read, 13 written, + 7 reals per contact written and read.
// ---------------------------------------------------------------------------------------------
// ALL (with NC = 8): this one launch steps every body, whatever its contact count -- a scene of a few ten thousand bodies is one
// wave per SIMD or less, where the tick costs the longest lane's chain once per LAUNCH: one launch beats two.
template <class T, bool EXT, int MINW, int NC, bool ALL = false>
__global__ __launch_bounds__(256, MINW) void step_contacts(T *S, T *So, int64_t n, StepParams<T> P, StepDiag *__restrict__ diag)
{
    static_assert(!ALL || NC == SC_MAXC, "the one-launch form holds every contact count");
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    int my_contacts = 0;
    double my_resid = 0.0;
    if (P.bp_check && P.bp_flags[BPF_VIOLATION] != 0u) return;      // the chunk will be rolled back whole
    if (P.gate != nullptr && *P.gate == 0u) return;
    const int cnt = (i < n && !(P.skip != nullptr && P.skip[i])) ? P.scount[i] : -1;
    // (a body with more contacts than the buffer holds is flagged, and stepped with the first SC_MAXC of them: what a caller
    //  who has switched the collision proof off -- nobody reads the flag then -- gets, and says so in include/dmx_batch.h)
    const bool mine = ALL ? cnt >= 0 : NC == 4 ? (cnt >= 0 && cnt <= 4) : (cnt > 4);
    if (NC == 4 || ALL) {
        const unsigned long long over = __ballot(cnt > SC_MAXC), need8 = __ballot(!ALL && cnt > 4 && cnt <= SC_MAXC && !P.have8);
        if ((over | need8) != 0ull && (threadIdx.x & 63) == 0 && P.bp_flags != nullptr) {
            if (over != 0ull) atomicOr(&P.bp_flags[BPF_NOFAST], 1u);
            if (need8 != 0ull) atomicOr(&P.bp_flags[BPF_NEED8], 1u);
            atomicOr(&P.bp_flags[BPF_VIOLATION], 1u);
        }
    } else if (__ballot(mine) == 0ull) return;                      // nobody here has 5..8 contacts
    if (mine) {
        V3<T> x = { S[slab_ix(C_POS + 0, i)], S[slab_ix(C_POS + 1, i)], S[slab_ix(C_POS + 2, i)] };
        if (P.bp_check) report_zone(zone_state(x.x - S[slab_ix(C_BPX, i)], x.z - S[slab_ix(C_BPZ, i)], S[slab_ix(C_BPSAFE, i)]), P.bp_flags);
        Q4<T> q = { S[slab_ix(C_QUAT + 0, i)], S[slab_ix(C_QUAT + 1, i)],
                    S[slab_ix(C_QUAT + 2, i)], S[slab_ix(C_QUAT + 3, i)] };
        V3<T> v = { S[slab_ix(C_LVEL + 0, i)], S[slab_ix(C_LVEL + 1, i)], S[slab_ix(C_LVEL + 2, i)] };
        V3<T> w = { S[slab_ix(C_AVEL + 0, i)], S[slab_ix(C_AVEL + 1, i)], S[slab_ix(C_AVEL + 2, i)] };
        const T mass = S[slab_ix(C_MASS, i)];
        const V3<T> Ib = { S[slab_ix(C_INERTIA + 0, i)], S[slab_ix(C_INERTIA + 1, i)],
                           S[slab_ix(C_INERTIA + 2, i)] };
        V3<T> facc = { T(0), T(0), T(0) }, tacc = { T(0), T(0), T(0) };
        if (EXT) {
            facc = { S[slab_ix(C_FORCE + 0, i)], S[slab_ix(C_FORCE + 1, i)], S[slab_ix(C_FORCE + 2, i)] };
            tacc = { S[slab_ix(C_TORQUE + 0, i)], S[slab_ix(C_TORQUE + 1, i)], S[slab_ix(C_TORQUE + 2, i)] };
        }

        const T h = P.h;
        const T invMass = T(1) / mass;
        M3<T> invIw;
        tick_head(q, w, mass, Ib, facc, tacc, P.g, h, P.gyro, invIw);
        const int nc = cnt > SC_MAXC ? SC_MAXC : cnt;
        my_contacts = nc;
        int ncu = 0;     // largest contact count among the wave's lanes stepped here (wave-uniform by construction)
#pragma unroll
        for (int k = 0; k < NC; k++)
            if (__ballot(nc > k) != 0ull) ncu = k + 1;

        if (ncu > 0) {
            constexpr int MAXR = 3 * NC;
            const int rpc = P.mu > 0 ? 3 : 1;
            const T hinv = T(1) / h;
            // v/h + M^-1 f
            const V3<T> tl = { fma_(facc.x, invMass, v.x * hinv), fma_(facc.y, invMass, v.y * hinv),
                               fma_(facc.z, invMass, v.z * hinv) };
            V3<T> ta = mulv(invIw, tacc);
            ta.x = fma_(w.x, hinv, ta.x); ta.y = fma_(w.y, hinv, ta.y); ta.z = fma_(w.z, hinv, ta.z);
            const T cfm = P.cfm * hinv;
            T rhs[MAXR], adcfm[MAXR], lam[MAXR];
            const T lo_f = -P.mu, hi_f = P.mu, hi_n = Limits<T>::inf();
            V3<T> Ja[MAXR], iMa[MAXR], Jl[MAXR], iMl[MAXR];      // J (angular, linear) times Ad, as J *= Ad leaves it; M^-1 J^T
#pragma unroll
            for (int r = 0; r < MAXR; r++) {      // rows of absent contacts stay zero
                rhs[r] = adcfm[r] = lam[r] = T(0);
                Ja[r] = { T(0), T(0), T(0) }; iMa[r] = { T(0), T(0), T(0) }; Jl[r] = { T(0), T(0), T(0) }; iMl[r] = { T(0), T(0), T(0) };
            }
#pragma unroll
            for (int k = 0; k < NC; k++) {
                if (k < ncu) {                    // (scalar branch; lanes with fewer contacts keep zero rows)
                    if (k < nc) {
                        const V3<T> cp = { P.sbuf[sc_ix(k, SC_POS + 0, i)], P.sbuf[sc_ix(k, SC_POS + 1, i)], P.sbuf[sc_ix(k, SC_POS + 2, i)] };
                        V3<T> dir[3];
                        dir[0] = { P.sbuf[sc_ix(k, SC_NORMAL + 0, i)], P.sbuf[sc_ix(k, SC_NORMAL + 1, i)], P.sbuf[sc_ix(k, SC_NORMAL + 2, i)] };
                        dir[1] = dir[2] = { T(0), T(0), T(0) };
                        if (rpc == 3) plane_space(dir[0], dir[1], dir[2]);
                        const V3<T> c1 = { cp.x - x.x, cp.y - x.y, cp.z - x.z };
#pragma unroll
                        for (int dnum = 0; dnum < 3; dnum++) {
                            const int r = 3 * k + dnum;
                            if (dnum < rpc) {
                                const V3<T> ja = cross(c1, dir[dnum]);
                                T c = T(0);
                                if (dnum == 0) {
                                    T depth = P.sbuf[sc_ix(k, SC_DEPTH, i)];
                                    if (depth < 0) depth = 0;
                                    c = (hinv * P.erp) * depth;
                                    if (P.surf_mode & SURF_BOUNCE) {
                                        const T outgoing = dot(dir[0], v) + dot(ja, w);
                                        if (P.bounce_vel >= 0 && (-outgoing) > P.bounce_vel) {
                                            const T newc = -P.bounce * outgoing;
                                            if (newc > c) c = newc;
                                        }
                                    }
                                }
                                T sum = dir[dnum].x * tl.x;
                                sum = fma_(dir[dnum].y, tl.y, sum); sum = fma_(dir[dnum].z, tl.z, sum);
                                sum = fma_(ja.x, ta.x, sum); sum = fma_(ja.y, ta.y, sum); sum = fma_(ja.z, ta.z, sum);
                                const T b = fma_(c, hinv, -sum);
                                const V3<T> iml = { invMass * dir[dnum].x, invMass * dir[dnum].y, invMass * dir[dnum].z };
                                const V3<T> ima = mulv(invIw, ja);
                                T s2 = iml.x * dir[dnum].x;
                                s2 = fma_(iml.y, dir[dnum].y, s2); s2 = fma_(iml.z, dir[dnum].z, s2);
                                s2 = fma_(ima.x, ja.x, s2); s2 = fma_(ima.y, ja.y, s2); s2 = fma_(ima.z, ja.z, s2);
                                const T ad = P.sor_w / (s2 + cfm);
                                Ja[r] = { ja.x * ad, ja.y * ad, ja.z * ad };
                                Jl[r] = { dir[dnum].x * ad, dir[dnum].y * ad, dir[dnum].z * ad };
                                iMa[r] = ima; iMl[r] = iml;
                                rhs[r] = b * ad;
                                adcfm[r] = ad * cfm;
                            }
                        }
                    }
                }
            }

            // ---- SOR-PGS: lambda = 0 start, rows in creation order; branch-free row update as in step_plane ----
            V3<T> fl = { T(0), T(0), T(0) }, fa = { T(0), T(0), T(0) };
            T rsum = T(0);
            // (the second copy of step_plane_body's sweep and dispatch, dmx_step_fused.hpp: change both.  FULL: as there -- every contact
            //  slot taken in every lane stepped here, friction rows present)
            auto sweep = [&](auto FAST, auto LAST, auto FULL) {
#pragma unroll
                for (int k = 0; k < NC; k++) {
                    if (decltype(FULL)::value || k < ncu) {
#pragma unroll
                        for (int dnum = 0; dnum < 3; dnum++) {
                            const int r = 3 * k + dnum;
                            if (decltype(FULL)::value || dnum < rpc) {
                                const T old = lam[r];
                                T delta = fma_(-old, adcfm[r], rhs[r]);
                                delta -= fma_(fa.z, Ja[r].z, fma_(fa.y, Ja[r].y, fma_(fa.x, Ja[r].x,
                                         fma_(fl.z, Jl[r].z, fma_(fl.y, Jl[r].y, fl.x * Jl[r].x)))));
                                const T nl = old + delta;
                                T nlam = nl;
                                if (dnum == 0 || !decltype(FAST)::value) {
                                    const T lo = dnum == 0 ? T(0) : lo_f, hi = dnum == 0 ? hi_n : hi_f;
                                    const bool below = nl < lo, above = nl > hi;
                                    nlam = below ? lo : (above ? hi : nl);
                                    delta = below ? lo - old : (above ? hi - old : delta);
                                }
                                lam[r] = nlam;
                                fl.x = fma_(delta, iMl[r].x, fl.x); fl.y = fma_(delta, iMl[r].y, fl.y);
                                fl.z = fma_(delta, iMl[r].z, fl.z);
                                fa.x = fma_(delta, iMa[r].x, fa.x); fa.y = fma_(delta, iMa[r].y, fa.y);
                                fa.z = fma_(delta, iMa[r].z, fa.z);
                                if (decltype(LAST)::value) rsum += tabs(delta);
                            }
                        }
                    }
                }
            };
            using std::true_type;
            using std::false_type;
            // FAST: friction rows are unbounded (mu = inf, the reference's surface, main.c:687): no friction clamp.  Lanes with
            // fewer contacts than the wave's count need no masking either way: their surplus rows are all zero, a zero row's
            // delta is exactly zero and leaves lambda and the accumulators as they are.
            const bool fast = !(P.mu < Limits<T>::inf());   // wave-uniform
            if (fast && ncu == NC && rpc == 3) {
                for (int it = 0; it + 1 < P.iters; it++) sweep(true_type{}, false_type{}, true_type{});
                if (P.iters > 0) sweep(true_type{}, true_type{}, true_type{});
            } else if (fast) {
                for (int it = 0; it + 1 < P.iters; it++) sweep(true_type{}, false_type{}, false_type{});
                if (P.iters > 0) sweep(true_type{}, true_type{}, false_type{});
            } else {
                for (int it = 0; it + 1 < P.iters; it++) sweep(false_type{}, false_type{}, false_type{});
                if (P.iters > 0) sweep(false_type{}, true_type{}, false_type{});
            }
            my_resid = (double)rsum;
            if (nc > 0) {        // v += h * (M^-1 J^T lambda)
                v.x = fma_(h, fl.x, v.x); v.y = fma_(h, fl.y, v.y); v.z = fma_(h, fl.z, v.z);
                w.x = fma_(h, fa.x, w.x); w.y = fma_(h, fa.y, w.y); w.z = fma_(h, fa.z, w.z);
            }
        }

        tick_tail(x, q, v, w, invMass, invIw, facc, tacc, h);
        pack_boundary(P, i, x, q, v, w);

        So[slab_ix(C_POS + 0, i)] = x.x; So[slab_ix(C_POS + 1, i)] = x.y; So[slab_ix(C_POS + 2, i)] = x.z;
        So[slab_ix(C_QUAT + 0, i)] = q.w; So[slab_ix(C_QUAT + 1, i)] = q.x;
        So[slab_ix(C_QUAT + 2, i)] = q.y; So[slab_ix(C_QUAT + 3, i)] = q.z;
        So[slab_ix(C_LVEL + 0, i)] = v.x; So[slab_ix(C_LVEL + 1, i)] = v.y; So[slab_ix(C_LVEL + 2, i)] = v.z;
        So[slab_ix(C_AVEL + 0, i)] = w.x; So[slab_ix(C_AVEL + 1, i)] = w.y; So[slab_ix(C_AVEL + 2, i)] = w.z;
        if (EXT) {
#pragma unroll
            for (int k = 0; k < 6; k++) S[slab_ix(C_FORCE + k, i)] = T(0);
        }
    }
    // ---- diagnostics: one slot per wave; the NC = 4 launch writes it, the NC = 8 launch behind it adds its lanes' share
    const int wc = wave_sum<int>(my_contacts);
    const double wr = wave_sum<double>(my_resid);
    if ((threadIdx.x & 63) == 0 && i < n) {
        StepDiag *d = &diag[(blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6];
        if (NC == 4 || ALL) { d->contacts = (unsigned long long)wc; d->residual = wr; }
        else { d->contacts += (unsigned long long)wc; d->residual += wr; }
    }
}

// ---------------------------------------------------------------------------------------------
// pack_transforms: GetTransformMat (main.c:602-622) per body: column-major 4x4 from pos + R(q).
// ---------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void pack_transforms(const T *__restrict__ S, int64_t stride, int64_t first,
                                                       int64_t count, T *__restrict__ out)
{
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t >= count) return;
    const int64_t i = first + t;
    const Q4<T> q = { S[slab_ix(C_QUAT + 0, i)], S[slab_ix(C_QUAT + 1, i)],
                      S[slab_ix(C_QUAT + 2, i)], S[slab_ix(C_QUAT + 3, i)] };
    const M3<T> R = quat_to_R(q);
    T *o = out + 16 * t;
    o[0] = R.m[0][0]; o[1] = R.m[1][0]; o[2] = R.m[2][0]; o[3] = T(0);
    o[4] = R.m[0][1]; o[5] = R.m[1][1]; o[6] = R.m[2][1]; o[7] = T(0);
    o[8] = R.m[0][2]; o[9] = R.m[1][2]; o[10] = R.m[2][2]; o[11] = T(0);
    o[12] = S[slab_ix(C_POS + 0, i)]; o[13] = S[slab_ix(C_POS + 1, i)];
    o[14] = S[slab_ix(C_POS + 2, i)]; o[15] = T(1);
}

// gather / scatter the 13 state reals of listed bodies (boundary exchange between GPUs)
// safe-zone test only, for slots the step kernels do not own (ghosts of a neighbour rank's boundary bodies)
template <class T>
__global__ __launch_bounds__(256) void check_zones(const T *__restrict__ S, int64_t first, int64_t count, uint32_t *flags)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int zs = 0;
    if (t < count) {
        const int64_t i = first + t;
        zs = zone_state(S[slab_ix(C_POS + 0, i)] - S[slab_ix(C_BPX, i)], S[slab_ix(C_POS + 2, i)] - S[slab_ix(C_BPZ, i)],
                        S[slab_ix(C_BPSAFE, i)]);
    }
    report_zone(zs, flags);
}

// Ghost refresh of the multi-GPU exchange, one launch per tick: the lower neighbour's rows (AoS, 13 reals per body) go
// to slots [first, first+count_lo), the upper neighbour's to the count_hi slots behind them; a null source leaves its
// range alone (no neighbour on that side).  With `check` the new (x,z) is tested against the slot's safe zone.
template <class T>
__global__ __launch_bounds__(256) void refresh_ghosts(T *__restrict__ S, int64_t first, int64_t count_lo,
                                                      const T *__restrict__ src_lo, int64_t count_hi,
                                                      const T *__restrict__ src_hi, int check, uint32_t *flags)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int zs = 0;
    if (t < count_lo + count_hi) {
        const T *src = t < count_lo ? src_lo : src_hi;
        if (src != nullptr) {
            const T *p = src + (t < count_lo ? t : t - count_lo) * C_MASS;
            const int64_t i = first + t;
#pragma unroll
            for (int c = 0; c < C_MASS; c++) S[slab_ix(c, i)] = p[c];
            if (check) zs = zone_state(p[0] - S[slab_ix(C_BPX, i)], p[2] - S[slab_ix(C_BPZ, i)], S[slab_ix(C_BPSAFE, i)]);
        }
    }
    if (check) report_zone(zs, flags);
}

// fill component c of every allocated body (pad included) with one value
template <class T>
__global__ __launch_bounds__(256) void fill_component(T *__restrict__ S, int c, T value, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) S[slab_ix(c, i)] = value;
}

// Rollback snapshot of the 13 state components (the first C_MASS reals x SLAB_TILE of every tile are one
// contiguous run): `packed` holds them tile after tile.  save: slab -> packed, else packed -> slab.
template <class T>
__global__ __launch_bounds__(256) void copy_state(T *__restrict__ S, T *__restrict__ packed, int64_t n_elems, bool save)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_elems) return;
    constexpr int64_t run = (int64_t)C_MASS * SLAB_TILE;
    const int64_t s = (t / run) * (int64_t)(C_COUNT * SLAB_TILE) + t % run;
    if (save) packed[t] = S[s];
    else      S[s] = packed[t];
}

// components [c0, c0+k) of bodies [first, first+count), slab to slab (the batch keeps two slabs of one layout)
template <class T>
__global__ __launch_bounds__(256) void copy_components(const T *__restrict__ from, T *__restrict__ to, int c0, int k,
                                                       int64_t first, int64_t count)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= count * k) return;
    const int c = (int)(t / count);
    const int64_t ix = slab_ix(c0 + c, first + (t - (int64_t)c * count));
    to[ix] = from[ix];
}

template <class T>
__global__ __launch_bounds__(256) void gather_bodies(const T *__restrict__ S, int64_t stride,
                                                     const int32_t *__restrict__ idx, int64_t count,
                                                     T *__restrict__ out)
{
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t >= count * C_MASS) return;
    const int64_t b = t / C_MASS;
    const int c = (int)(t - b * C_MASS);
    out[t] = S[slab_ix(c, idx[b])];
}
template <class T>
__global__ __launch_bounds__(256) void scatter_bodies(T *__restrict__ S, int64_t stride,
                                                      const int32_t *__restrict__ idx, int64_t count,
                                                      const T *__restrict__ in)
{
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t >= count * C_MASS) return;
    const int64_t b = t / C_MASS;
    const int c = (int)(t - b * C_MASS);
    S[slab_ix(c, idx[b])] = in[t];
}

// host-order rows (n x k, array of structs) <-> the slab's component tiles, used by upload/download through a staging buffer
template <class T>
__global__ __launch_bounds__(256) void aos_to_soa(T *__restrict__ S, int64_t stride, int comp0, int k,
                                                  int64_t first, int64_t count, const T *__restrict__ aos)
{
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t >= count * k) return;
    const int64_t b = t / k;
    const int c = (int)(t - b * k);
    S[slab_ix(comp0 + c, first + b)] = aos[t];
}
template <class T>
__global__ __launch_bounds__(256) void soa_to_aos(const T *__restrict__ S, int64_t stride, int comp0, int k,
                                                  int64_t first, int64_t count, T *__restrict__ aos)
{
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t >= count * k) return;
    const int64_t b = t / k;
    const int c = (int)(t - b * k);
    aos[t] = S[slab_ix(comp0 + c, first + b)];
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
static inline unsigned blocks_for(int64_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }
constexpr int64_t kOneLaunchBodies = 256 * 4 * 64;

template <class T>
hipError_t launch_step(T *S, T *So, const uint8_t *gtype, int64_t stride, int64_t n, const StepParams<T> &P, bool ext,
                       StepDiag *diag, hipStream_t st, int rev, int fix_mode, uint32_t *fix_words, bool torque_free, int64_t *tf_stats,
                       bool lean_kernel, int64_t *lk_stats)
{
    if (P.n_static > 0 && P.sbuf != nullptr) {
        // bodies at static geometry: narrowphase against the plane and the static boxes, then the fused solve + integrate
        const hipError_t e = launch_np_static<T>(S, gtype, n, P, st);
        if (e != hipSuccess) return e;
        const unsigned grid = blocks_for(n, 256);
        // up to one wave per SIMD of the chip (256 CUs x 4 SIMDs x 64 lanes): the tick is the longest lane's chain per launch
        if (P.have8 && n <= kOneLaunchBodies && sizeof(T) == 4) {
            if (ext) hipLaunchKernelGGL((step_contacts<T, true, 1, 8, true>), dim3(grid), dim3(256), 0, st, S, So, n, P, diag);
            else     hipLaunchKernelGGL((step_contacts<T, false, 1, 8, true>), dim3(grid), dim3(256), 0, st, S, So, n, P, diag);
            return hipGetLastError();
        }
        if (ext) hipLaunchKernelGGL((step_contacts<T, true, 1, 4>), dim3(grid), dim3(256), 0, st, S, So, n, P, diag);
        else if (sizeof(T) == 4) hipLaunchKernelGGL((step_contacts<T, false, 2, 4>), dim3(grid), dim3(256), 0, st, S, So, n, P, diag);
        else hipLaunchKernelGGL((step_contacts<T, false, 1, 4>), dim3(grid), dim3(256), 0, st, S, So, n, P, diag);
        if (P.have8) {
            if (ext) hipLaunchKernelGGL((step_contacts<T, true, 1, 8>), dim3(grid), dim3(256), 0, st, S, So, n, P, diag);
            else     hipLaunchKernelGGL((step_contacts<T, false, 1, 8>), dim3(grid), dim3(256), 0, st, S, So, n, P, diag);
        }
    } else if (!P.plane_on) {
        // One body per lane.  On the tiled slab a wave's loads (17, or 13 when the constants are arguments) already cover one
        // contiguous run, so wider per-lane loads buy nothing, and one body keeps the f32 kernel at 7 waves/SIMD (71 VGPRs
        // with every load and store, 72 in the default instantiation below): measured, on the kernel moving all 30 reals,
        // 21.1 / 22.2 / 22.4 us per tick for 1 / 2 / 4 bodies per lane at 1 Mi f32 bodies
        // (profiles/r01_integrate_free_tiled_sweep.txt).  Pad bodies up to `stride` are valid memory.
        // The grid is rounded up to a multiple of 8 workgroups (the surplus ones leave at the kernel's i < n): the sweep order
        // (dmx_sweep.hpp) is defined on such grids, and workgroup b of every launch then has the same b % 8, whether the
        // dispatcher starts its round-robin over the XCDs anew at each launch or carries it on.  `rev` is this launch's direction.
        const unsigned grid = sweep_grid(blocks_for(n, 256));
        // what the result does not need (the kernel's header): store elision, and constants as arguments when the batch's are uniform.
        // The constants' scalars cost the f32 one-tick kernel three registers (71 -> 74 VGPRs = 6 waves per SIMD): a launch bound
        // of 7 waves (MWU) makes the allocator fit them into the 72 that 7 waves allow, without scratch; the kernels with force
        // accumulators or many ticks would spill under that bound and keep the default one.  The many-ticks-per-launch
        // kernel (VALU-bound, one store per `ticks` ticks) keeps its unconditional stores: the copy of the loaded state would
        // cost it a wave per SIMD (78 -> 91 VGPRs, 6 -> 5 waves) for a store it rarely issues, while the constants as arguments
        // cost it none (78 -> 79); a build with the elision in it measured the same within the spread at 32 ticks per launch
        // (profiles/ab_elision_multi.txt).  DESIGN.md section 3 has the table.  (Since the constants' quotients come from the host the
        // f32 kernels with OPT_UNI need 65 to 68 VGPRs and the bound no longer binds them; it stays, and also holds the kernel with
        // FIX that loads its constants, which without its gate and skip tests would take 73 -- profiles/launch_consts_resources.txt.)
        constexpr int MWU = sizeof(T) == 4 ? 7 : 1;
        // Constants as arguments come with their quotients (dmx_launch_consts.hpp), which the instantiations with OPT_UNI read where
        // the others divide per lane.  Where the rule refuses them -- a zero, an infinity or a NaN among mass, inertia and h, or a
        // reciprocal that is not finite -- the launch drops OPT_UNI and loads the constants per lane, as a batch with mixed ones does.
        const T tf_Ib[3] = { P.uni_inertia.x, P.uni_inertia.y, P.uni_inertia.z }, tf_g[3] = { P.g.x, P.g.y, P.g.z };
        const LaunchConsts<T> lc = launch_consts<T>(P.uni_mass, tf_Ib, P.h);
        const int opt = (P.elide & OPT_ELIDE) | ((P.elide & OPT_UNI) && P.uni && lc.on ? OPT_UNI : 0);
        // the short tick of a body without torque (dmx_torque_free.hpp has the rule): on -- the instantiations with TF -- or off, with the
        // launch's constants
        const TorqueFree<T> tf = torque_free_plan<T>(torque_free, (opt & OPT_UNI) != 0, ext, P.gyro, P.uni_mass, tf_Ib, P.h, tf_g);
        if (tf_stats != nullptr) tf_stats[tf.on ? 0 : 1]++;      // contact-free launches with / without the short tick built in
        auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, st, S, So, n, P, rev & 1, fix_mode, fix_words, tf, lc); };
        // an establishing or lean launch (dmx_fixed.hpp; the caller has asked the batch's record) is one of the two instantiations
        // with the fixed-axis mode built in; every other launch is the kernel it always was
        if (fix_mode != FIX_OFF) {
            // (no gate, no skip mask: the instantiations with FIX do not read either pointer and rely on this refusal)
            if (P.ticks > 1 || ext || !(opt & OPT_ELIDE) || fix_words == nullptr || P.skip != nullptr || P.gate != nullptr) return hipErrorInvalidValue;
            // a lean launch has not loaded every pos.x / pos.z: it cannot fill another slab, test safe zones or pack the boundary
            if (fix_mode == FIX_LEAN && (So != S || P.bp_check != 0 || P.pack_out != nullptr)) return hipErrorInvalidValue;
            // A lean launch with the constants as arguments and the short tick on -- all decided above -- is the straight-line kernel
            // (integrate_free_lean), unless the batch's switch is off: what a wavefront of it reads ahead of its loads is LeanHot alone.
            // The refusals above hold for it as they stand: in place, one tick, no accumulators, no zones, no pack, no gate, no skip mask.
            const bool lean = lean_kernel && fix_mode == FIX_LEAN && opt == 3 && tf.on;
            if (lk_stats != nullptr) lk_stats[lean ? 0 : 1]++;
            if (lean) {
                const LeanHot<T> hot = { n, grid, rev & 1, S, fix_words, P.h, tf.hm, tf.mg[1] };
                hipLaunchKernelGGL((integrate_free_lean<T>), dim3(grid), dim3(256), 0, st, hot, P, tf, lc);
            }
            else if (opt == 3 && tf.on) launch(integrate_free<T, false, MWU, false, 3, true, true>);
            else if (opt == 3) launch(integrate_free<T, false, MWU, false, 3, true>);
            else launch(integrate_free<T, false, MWU, false, 1, true>);
        } else if (P.ticks > 1) {
            if (lk_stats != nullptr) lk_stats[1]++;
            if ((opt & OPT_UNI) && tf.on) launch(integrate_free<T, false, 1, true, OPT_UNI, false, true>);
            else if (opt & OPT_UNI) launch(integrate_free<T, false, 1, true, OPT_UNI>);
            else launch(integrate_free<T, false, 1, true, 0>);
        } else if (ext) {
            if (lk_stats != nullptr) lk_stats[1]++;
            if (opt == 3) launch(integrate_free<T, true, 1, false, 3>);
            else if (opt == 2) launch(integrate_free<T, true, 1, false, 2>);
            else if (opt == 1) launch(integrate_free<T, true, 1, false, 1>);
            else launch(integrate_free<T, true, 1, false, 0>);
        } else {
            if (lk_stats != nullptr) lk_stats[1]++;
            if (opt == 3 && tf.on) launch(integrate_free<T, false, MWU, false, 3, false, true>);
            else if (opt == 2 && tf.on) launch(integrate_free<T, false, MWU, false, 2, false, true>);
            else if (opt == 3) launch(integrate_free<T, false, MWU, false, 3>);
            else if (opt == 2) launch(integrate_free<T, false, MWU, false, 2>);
            else if (opt == 1) launch(integrate_free<T, false, 1, false, 1>);
            else launch(integrate_free<T, false, 1, false, 0>);
        }
    } else {
        const unsigned grid = blocks_for(n, 256);
        // convex bodies: their plane contacts first (one wavefront per body), then the fused step with 8 contact slots
        if (P.hull_n > 0 && P.cbuf != nullptr) {
            const hipError_t e = launch_np_convex_plane<T>(S, gtype, n, P, st);
            if (e != hipSuccess) return e;
            if (ext) hipLaunchKernelGGL((step_plane<T, true, 1, CONVEX_MAXC>), dim3(grid), dim3(256), 0, st, S, So, gtype, stride, n, P, diag);
            else     hipLaunchKernelGGL((step_plane<T, false, 1, CONVEX_MAXC>), dim3(grid), dim3(256), 0, st, S, So, gtype, stride, n, P, diag);
        } else {
            constexpr int MW = sizeof(T) == 4 ? 2 : 1;
            if (ext) hipLaunchKernelGGL((step_plane<T, true, MW, 4>), dim3(grid), dim3(256), 0, st, S, So, gtype, stride, n, P, diag);
            else     hipLaunchKernelGGL((step_plane<T, false, MW, 4>), dim3(grid), dim3(256), 0, st, S, So, gtype, stride, n, P, diag);
        }
    }
    return hipGetLastError();
}

template <class T>
hipError_t launch_pack_transforms(const T *S, int64_t stride, int64_t first, int64_t count, T *out, hipStream_t st)
{
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL((pack_transforms<T>), dim3(blocks_for(count, 256)), dim3(256), 0, st, S, stride, first, count, out);
    return hipGetLastError();
}
template <class T>
hipError_t launch_check_zones(const T *S, int64_t first, int64_t count, uint32_t *flags, hipStream_t st)
{
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL((check_zones<T>), dim3(blocks_for(count, 256)), dim3(256), 0, st, S, first, count, flags);
    return hipGetLastError();
}

template <class T>
hipError_t launch_refresh_ghosts(T *S, int64_t first, int64_t count_lo, const T *src_lo, int64_t count_hi, const T *src_hi,
                                 int check, uint32_t *flags, hipStream_t st)
{
    if (count_lo + count_hi <= 0) return hipSuccess;
    hipLaunchKernelGGL((refresh_ghosts<T>), dim3(blocks_for(count_lo + count_hi, 256)), dim3(256), 0, st, S, first, count_lo,
                       src_lo, count_hi, src_hi, check, flags);
    return hipGetLastError();
}

template <class T>
hipError_t launch_fill_component(T *S, int c, T value, int64_t n, hipStream_t st)
{
    hipLaunchKernelGGL((fill_component<T>), dim3(blocks_for(n, 256)), dim3(256), 0, st, S, c, value, n);
    return hipGetLastError();
}

template <class T>
hipError_t launch_copy_state(T *S, T *packed, int64_t n_bodies, bool save, hipStream_t st)
{
    const int64_t n_elems = (n_bodies + SLAB_TILE - 1) / SLAB_TILE * C_MASS * SLAB_TILE;
    hipLaunchKernelGGL((copy_state<T>), dim3(blocks_for(n_elems, 256)), dim3(256), 0, st, S, packed, n_elems, save);
    return hipGetLastError();
}

template <class T>
hipError_t launch_copy_components(const T *from, T *to, int c0, int k, int64_t first, int64_t count, hipStream_t st)
{
    if (count <= 0 || k <= 0) return hipSuccess;
    hipLaunchKernelGGL((copy_components<T>), dim3(blocks_for(count * k, 256)), dim3(256), 0, st, from, to, c0, k, first, count);
    return hipGetLastError();
}

template <class T>
hipError_t launch_gather(const T *S, int64_t stride, const int32_t *idx, int64_t count, T *out, hipStream_t st)
{
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL((gather_bodies<T>), dim3(blocks_for(count * C_MASS, 256)), dim3(256), 0, st, S, stride, idx, count, out);
    return hipGetLastError();
}
template <class T>
hipError_t launch_scatter(T *S, int64_t stride, const int32_t *idx, int64_t count, const T *in, hipStream_t st)
{
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL((scatter_bodies<T>), dim3(blocks_for(count * C_MASS, 256)), dim3(256), 0, st, S, stride, idx, count, in);
    return hipGetLastError();
}
template <class T>
hipError_t launch_aos_to_soa(T *S, int64_t stride, int comp0, int k, int64_t first, int64_t count, const T *aos,
                             hipStream_t st)
{
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL((aos_to_soa<T>), dim3(blocks_for(count * k, 256)), dim3(256), 0, st, S, stride, comp0, k, first, count, aos);
    return hipGetLastError();
}
template <class T>
hipError_t launch_soa_to_aos(const T *S, int64_t stride, int comp0, int k, int64_t first, int64_t count, T *aos,
                             hipStream_t st)
{
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL((soa_to_aos<T>), dim3(blocks_for(count * k, 256)), dim3(256), 0, st, S, stride, comp0, k, first, count, aos);
    return hipGetLastError();
}

#define DMX_INSTANTIATE(T)                                                                                         \
    template hipError_t launch_step<T>(T *, T *, const uint8_t *, int64_t, int64_t, const StepParams<T> &, bool,   \
                                       StepDiag *, hipStream_t, int, int, uint32_t *, bool, int64_t *, bool, int64_t *);                                   \
    template hipError_t launch_pack_transforms<T>(const T *, int64_t, int64_t, int64_t, T *, hipStream_t);         \
    template hipError_t launch_gather<T>(const T *, int64_t, const int32_t *, int64_t, T *, hipStream_t);          \
    template hipError_t launch_scatter<T>(T *, int64_t, const int32_t *, int64_t, const T *, hipStream_t);         \
    template hipError_t launch_aos_to_soa<T>(T *, int64_t, int, int, int64_t, int64_t, const T *, hipStream_t);    \
    template hipError_t launch_soa_to_aos<T>(const T *, int64_t, int, int, int64_t, int64_t, T *, hipStream_t);     \
    template hipError_t launch_fill_component<T>(T *, int, T, int64_t, hipStream_t);                                \
    template hipError_t launch_copy_state<T>(T *, T *, int64_t, bool, hipStream_t);                                 \
    template hipError_t launch_copy_components<T>(const T *, T *, int, int, int64_t, int64_t, hipStream_t);         \
    template hipError_t launch_check_zones<T>(const T *, int64_t, int64_t, uint32_t *, hipStream_t);               \
    template hipError_t launch_refresh_ghosts<T>(T *, int64_t, int64_t, const T *, int64_t, const T *, int, uint32_t *, hipStream_t);
DMX_INSTANTIATE(float)
DMX_INSTANTIATE(double)

// HIP loads a translation unit's code object at the first launch of one of its kernels -- a couple of milliseconds each, which an
// interactive caller would meet as a hitch at the first tick that needs the exact pipeline.  dmxBatchCreate asks for one
// kernel's attributes per unit instead (dmx_preload_code, dmx_batch.cpp): the load happens there.
hipError_t dmx_touch_kernels(int real_bytes)
{
    // (the unit's code object, and -- what costs more -- each kernel's own first-use set-up: every kernel an exact tick or a fused
    //  tick may launch, in the batch's precision)
    hipFuncAttributes a;
    hipError_t e = hipSuccess;
    auto touch = [&](const void *k) { const hipError_t r = hipFuncGetAttributes(&a, k); if (r != hipSuccess) e = r; };
    if (real_bytes == 4) {
        touch((const void *)&integrate_free<float, false, 1, false>);
        touch((const void *)&integrate_free<float, false, 7, false, 3>);
        touch((const void *)&integrate_free<float, false, 7, false, 3, true>);
        touch((const void *)&integrate_free<float, false, 7, false, 3, false, true>);
        touch((const void *)&integrate_free<float, false, 7, false, 3, true, true>);
        touch((const void *)&integrate_free_lean<float>);
        touch((const void *)&step_plane<float, false, 2, 4>);
        touch((const void *)&step_contacts<float, false, 1, 8, true>);
        touch((const void *)&check_zones<float>);
        touch((const void *)&copy_components<float>);
    } else {
        touch((const void *)&integrate_free<double, false, 1, false>);
        touch((const void *)&integrate_free<double, false, 1, false, 3>);
        touch((const void *)&integrate_free<double, false, 1, false, 3, true>);
        touch((const void *)&integrate_free<double, false, 1, false, 3, false, true>);
        touch((const void *)&integrate_free<double, false, 1, false, 3, true, true>);
        touch((const void *)&integrate_free_lean<double>);
        touch((const void *)&step_plane<double, false, 1, 4>);
        touch((const void *)&step_contacts<double, false, 1, 8, true>);
        touch((const void *)&check_zones<double>);
        touch((const void *)&copy_components<double>);
    }
    return e;
}

}  // namespace dmx
