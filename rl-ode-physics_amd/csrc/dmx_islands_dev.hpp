// dmx_islands_dev.hpp -- the island kernels' bodies as device functions: one lane per island (solve_islands_body, and the
// one-body forms solve_singles_body / solve_singles_lds_body), one workgroup per island (solve_island_wg_body).  The kernels of
// dmx_islands.hip are thin wrappers; the single-launch tick of small worlds (dmx_small.hip) calls the same functions.
#pragma once

#include <hip/hip_runtime.h>
#include "dmx_internal.hpp"
#include "dmx_exact.hpp"
#include "dmx_math.hpp"
#include "dmx_step_fused.hpp"
#include "dmx_island_rows.hpp"

namespace dmx {

// ================================================================================ one lane per single-body island, rows in registers
// A body touching static geometry only (the ground plane, static boxes) is an island of its own: all its rows share the one
// body, so the sweep is a pure chain -- a wavefront per island (solve_island_wg) would run one lane at a time.  Here a LANE
// owns the island: up to SINGLE_MAXC contacts x 3 rows live in its registers (no row traffic at all), 64 islands per wave.
// stage_body, body_tmp and finish_body are the general island step's own; contact_rows is single_contact / single_contact_row
// (dmx_island_rows.hpp: the second body absent), row_setup and row_sor are restated here
// with the second body absent, held to the general path bit for bit by tests/test_gpu_static.py and tests/test_gpu_parity.py.  (What a box resting on the reference's floor, main.c:115, costs per tick.)
constexpr int SINGLE_MAXC = 4;          // rows in registers (solve_singles)
constexpr int SINGLE_MAXC_LDS = 8;      // rows in LDS (solve_singles_lds): a convex hull's eight contacts with the floor

template <class T> __device__ __forceinline__ bool island_is_single(const IslandSet<T> &I, int isl)
{
    const int nb = I.body_off[isl + 1] - I.body_off[isl], nc = I.con_off[isl + 1] - I.con_off[isl];
    // (an island's articulation units come first: one body on a joint to the world is not the one-body forms' island)
    return nb == 1 && nc >= 1 && nc <= SINGLE_MAXC_LDS && !contact_is_unit(I, I.con_off[isl]);
}

template <class T> struct RowS { T J[6], iMJ[6], rhs, ad, lam; };

template <class T>
__device__ __forceinline__ void solve_singles_body(T *__restrict__ S, const uint8_t *__restrict__ bflags, int64_t stride,
                                                   const IslandSet<T> &I, const StepParams<T> &P, StepDiag *__restrict__ diag, int isl)
{
    if (isl >= I.n_islands || !island_is_single(I, isl)) return;
    const T h = P.h, hinv = T(1) / h;
    const int s = I.bodies[I.body_off[isl]];
    const int c0 = I.con_off[isl], nc = I.con_off[isl + 1] - c0;
    if (nc > SINGLE_MAXC) return;                             // five to eight contacts: solve_singles_lds
    T b[BW_COUNT];
    stage_body(S, bflags, stride, I, P, b, s, 0);
    const V3<T> x1 = ldS(S, stride, C_POS, s), v1 = ldS(S, stride, C_LVEL, s), w1 = ldS(S, stride, C_AVEL, s);
    constexpr int MAXR = 3 * SINGLE_MAXC;
    RowS<T> row[MAXR];
    bool valid[MAXR];
    T lo_f[SINGLE_MAXC], hi_f[SINGLE_MAXC];           // friction bounds of contact c (normal rows: [0, inf))
#pragma unroll
    for (int c = 0; c < SINGLE_MAXC; c++) {
#pragma unroll
        for (int d = 0; d < 3; d++) valid[3 * c + d] = false;
        lo_f[c] = hi_f[c] = T(0);
        if (c < nc) {
            size_t gi; int mode, rpc;
            V3<T> c1, dir[3];
            single_contact(I, P, c0 + c, x1, gi, c1, mode, rpc, dir, lo_f[c], hi_f[c]);
#pragma unroll
            for (int dnum = 0; dnum < 3; dnum++) {
                if (dnum < rpc) {
                    RowS<T> &r = row[3 * c + dnum];
                    valid[3 * c + dnum] = true;
                    single_contact_row(I, P, c0 + c, gi, mode, dnum == 0, c1, dir[dnum], v1, w1, hinv, r.J, r.rhs, r.ad);      // (c and cfm for now)
                    r.lam = T(0);
                }
            }
        }
    }
    body_tmp(S, stride, b, s, hinv);
    // ---- row_setup
#pragma unroll
    for (int i = 0; i < MAXR; i++) {
        if (valid[i]) {
            RowS<T> &r = row[i];
            T sum = T(0);
#pragma unroll
            for (int j = 0; j < 6; j++) sum = fma_(r.J[j], b[BW_TMP + j], sum);
            r.rhs = fma_(r.rhs, hinv, -sum);
            r.ad *= hinv;
#pragma unroll
            for (int j = 0; j < 3; j++) r.iMJ[j] = b[BW_INVM] * r.J[j];
            const V3<T> ja1 = { r.J[3], r.J[4], r.J[5] };
            r.iMJ[3] = dot3p(b + BW_INVI + 0, ja1); r.iMJ[4] = dot3p(b + BW_INVI + 3, ja1); r.iMJ[5] = dot3p(b + BW_INVI + 6, ja1);
            T s2 = T(0);
#pragma unroll
            for (int j = 0; j < 6; j++) s2 = fma_(r.iMJ[j], r.J[j], s2);
            const T cfm = r.ad;
            const T ad = P.sor_w / (s2 + cfm);
#pragma unroll
            for (int j = 0; j < 6; j++) r.J[j] *= ad;
            r.rhs *= ad;
            r.ad = ad * cfm;
        }
    }
    // ---- the sweeps (row_sor), rows in creation order
    double resid = 0.0;
    T *fc = b + BW_FC;
    for (int it = 0; it < P.iters; it++) {
        const bool last = (it == P.iters - 1);
#pragma unroll
        for (int i = 0; i < MAXR; i++) {
            if (valid[i]) {
                RowS<T> &r = row[i];
                const T old = r.lam;
                T delta = fma_(-old, r.ad, r.rhs);
                delta -= fma_(fc[5], r.J[5], fma_(fc[4], r.J[4], fma_(fc[3], r.J[3], fma_(fc[2], r.J[2], fma_(fc[1], r.J[1], fc[0] * r.J[0])))));
                const T lo = (i % 3 == 0) ? T(0) : lo_f[i / 3], hi = (i % 3 == 0) ? Limits<T>::inf() : hi_f[i / 3];
                const T nl = old + delta;
                if (nl < lo) { delta = lo - old; r.lam = lo; }
                else if (nl > hi) { delta = hi - old; r.lam = hi; }
                else r.lam = nl;
#pragma unroll
                for (int j = 0; j < 6; j++) fc[j] = fma_(delta, r.iMJ[j], fc[j]);
                if (last) resid += (double)tabs(delta);
            }
        }
    }
    finish_body(S, bflags, stride, b, s, true, h, I.damping);
    atomicAdd(&diag->contacts, (unsigned long long)nc);
    atomicAdd(&diag->residual, resid);
}

// The same island shape with five to eight contacts (a convex hull on the floor: up to 24 rows): too many rows for a lane's
// registers, so their J and M^-1 J^T live in LDS, one column per lane (field f of row r of lane l at
// [(r * RS_FIELDS + f) * lanes + l]: a wavefront's access to one field is one conflict-free LDS row); rhs, Ad cfm and lambda
// stay in registers.  A row update is one batch of twelve independent LDS reads, then arithmetic: the same sequence once more.
enum : int { RS_J = 0, RS_IMJ = 6, RS_FIELDS = 12 };      // per row in LDS: J (scaled by Ad) and M^-1 J^T; rhs, Ad cfm, lambda stay in registers

// (lanes islands share the launch's dynamic LDS, lane `lane` of them this one: island isl)
template <class T>
__device__ __forceinline__ void solve_singles_lds_body(T *__restrict__ S, const uint8_t *__restrict__ bflags, int64_t stride,
                                                       const IslandSet<T> &I, const StepParams<T> &P, StepDiag *__restrict__ diag,
                                                       int isl, int lanes, int lane)
{
    extern __shared__ __align__(16) unsigned char rs_raw[];
    T *rs = reinterpret_cast<T *>(rs_raw);
    constexpr int MAXR = 3 * SINGLE_MAXC_LDS;
    if (isl >= I.n_islands || !island_is_single(I, isl)) return;
    const int c0 = I.con_off[isl], nc = I.con_off[isl + 1] - c0;
    if (nc <= SINGLE_MAXC) return;                            // solve_singles has it
    const T h = P.h, hinv = T(1) / h;
    const int s = I.bodies[I.body_off[isl]];
    T b[BW_COUNT];
    stage_body(S, bflags, stride, I, P, b, s, 0);
    const V3<T> x1 = ldS(S, stride, C_POS, s), v1 = ldS(S, stride, C_LVEL, s), w1 = ldS(S, stride, C_AVEL, s);
    auto at = [&](int r, int f) -> T & { return rs[(size_t)(r * RS_FIELDS + f) * lanes + lane]; };
    unsigned valid = 0;                                       // bit r: slot r (= 3 * contact + direction) holds a row
    T lo_f[SINGLE_MAXC_LDS], hi_f[SINGLE_MAXC_LDS];
    T rhsr[MAXR], adr[MAXR], lamr[MAXR];
#pragma unroll
    for (int q = 0; q < MAXR; q++) rhsr[q] = adr[q] = lamr[q] = T(0);
#pragma unroll
    for (int c = 0; c < SINGLE_MAXC_LDS; c++) {
        lo_f[c] = hi_f[c] = T(0);
        if (c >= nc) continue;
        size_t gi; int mode, rpc;
        V3<T> c1, dir[3];
        single_contact(I, P, c0 + c, x1, gi, c1, mode, rpc, dir, lo_f[c], hi_f[c]);
#pragma unroll
        for (int dnum = 0; dnum < 3; dnum++) {
            if (dnum >= rpc) continue;
            const int r = 3 * c + dnum;
            valid |= 1u << r;
            T J[6], cval, cfm;
            single_contact_row(I, P, c0 + c, gi, mode, dnum == 0, c1, dir[dnum], v1, w1, hinv, J, cval, cfm);
            for (int j = 0; j < 6; j++) at(r, RS_J + j) = J[j];
#pragma unroll
            for (int q = 0; q < MAXR; q++) if (q == r) { rhsr[q] = cval; adr[q] = cfm; }      // (static indices keep the arrays in registers)
        }
    }
    body_tmp(S, stride, b, s, hinv);
#pragma unroll
    for (int i = 0; i < MAXR; i++) {                          // row_setup
        if (!(valid >> i & 1u)) continue;
        T J[6], iMJ[6];
#pragma unroll
        for (int j = 0; j < 6; j++) J[j] = at(i, RS_J + j);
        T sum = T(0);
#pragma unroll
        for (int j = 0; j < 6; j++) sum = fma_(J[j], b[BW_TMP + j], sum);
        T rhs = fma_(rhsr[i], hinv, -sum);
        const T cfm = adr[i] * hinv;
        for (int j = 0; j < 3; j++) iMJ[j] = b[BW_INVM] * J[j];
        const V3<T> ja1 = { J[3], J[4], J[5] };
        iMJ[3] = dot3p(b + BW_INVI + 0, ja1); iMJ[4] = dot3p(b + BW_INVI + 3, ja1); iMJ[5] = dot3p(b + BW_INVI + 6, ja1);
        T s2 = T(0);
        for (int j = 0; j < 6; j++) s2 = fma_(iMJ[j], J[j], s2);
        const T ad = P.sor_w / (s2 + cfm);
#pragma unroll
        for (int j = 0; j < 6; j++) { at(i, RS_J + j) = J[j] * ad; at(i, RS_IMJ + j) = iMJ[j]; }
        rhs *= ad;
        rhsr[i] = rhs;
        adr[i] = ad * cfm;
        lamr[i] = T(0);
    }
    double resid = 0.0;
    T *fc = b + BW_FC;
    // One sweep (row_sor, rows in creation order).  A row's twelve LDS words do not depend on the rows before it: they are
    // fetched, in one batch of independent reads, while the row before is being updated -- the chain of updates never waits
    // for LDS.  (Slots without a row are fetched too and not used.)  LAST: the final sweep also sums |delta lambda|.
    auto sweep = [&](auto LAST) {
        T rw[RS_FIELDS], nx[RS_FIELDS];
#pragma unroll
        for (int f = 0; f < RS_FIELDS; f++) rw[f] = at(0, f);
#pragma unroll
        for (int i = 0; i < MAXR; i++) {
            if (i + 1 < MAXR) {
#pragma unroll
                for (int f = 0; f < RS_FIELDS; f++) nx[f] = at(i + 1, f);
            }
            if (valid >> i & 1u) {
                const T old = lamr[i];
                T delta = fma_(-old, adr[i], rhsr[i]);
                delta -= fma_(fc[5], rw[RS_J + 5], fma_(fc[4], rw[RS_J + 4], fma_(fc[3], rw[RS_J + 3],
                         fma_(fc[2], rw[RS_J + 2], fma_(fc[1], rw[RS_J + 1], fc[0] * rw[RS_J + 0])))));
                const T lo = (i % 3 == 0) ? T(0) : lo_f[i / 3], hi = (i % 3 == 0) ? Limits<T>::inf() : hi_f[i / 3];
                const T nl = old + delta;
                T lam = nl;
                if (nl < lo) { delta = lo - old; lam = lo; }
                else if (nl > hi) { delta = hi - old; lam = hi; }
                lamr[i] = lam;
#pragma unroll
                for (int j = 0; j < 6; j++) fc[j] = fma_(delta, rw[RS_IMJ + j], fc[j]);
                if (decltype(LAST)::value) resid += (double)tabs(delta);
            }
            if (i + 1 < MAXR) {
#pragma unroll
                for (int f = 0; f < RS_FIELDS; f++) rw[f] = nx[f];
            }
            // (one row ahead and no further: left to itself the scheduler hoists every fetch of the unrolled sweep to its top,
            //  288 registers of them)
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    for (int it = 0; it + 1 < P.iters; it++) sweep(std::false_type{});
    if (P.iters > 0) sweep(std::true_type{});
    finish_body(S, bflags, stride, b, s, true, h, I.damping);
    atomicAdd(&diag->contacts, (unsigned long long)nc);
    atomicAdd(&diag->residual, resid);
}

// ================================================================================ one lane per island
// FB: a tick made with feedback on (dmxBatchSetFeedback) -- row_setup also leaves what entry_feedback needs.  An instantiation of
// its own, here and in solve_island_wg_body, so that a tick without feedback runs the code it ran before feedback existed.
// APX: a tick with pyramid rows (DMX_CONTACT_APPROX1) -- contact_rows marks them, row_sor makes their bounds from the normal row's
// multiplier.  Again an instantiation of its own, here and in solve_island_wg_body; the host launches it with FB's store on, so one
// kernel serves such a tick with feedback on or off.
template <class T, bool FB = false, bool APX = false>
__device__ __forceinline__ void solve_islands_body(T *__restrict__ S, const uint8_t *__restrict__ bflags,
                                                   int64_t stride, const IslandSet<T> &I, const StepParams<T> &P,
                                                   StepDiag *__restrict__ diag, int isl)
{
    if (isl >= I.n_islands) return;
    if (I.big != nullptr && I.big[isl] >= 0) return;          // a workgroup owns this one (solve_island_wg)
    if (I.singles && island_is_single(I, isl)) return;        // one body, a few static contacts: solve_singles
    const T h = P.h, hinv = T(1) / h;
    const int b0 = I.body_off[isl], nb = I.body_off[isl + 1] - b0;
    const int c0 = I.con_off[isl], nc = I.con_off[isl + 1] - c0;
    const int r0 = I.row_off[isl];
    T *bs = I.bscr + (size_t)b0 * BW_COUNT;
    T *rows = I.rows + (size_t)r0 * RW_COUNT;
    int *jb = I.rowjb + 2 * (size_t)r0;

    for (int k = 0; k < nb; k++) stage_body(S, bflags, stride, I, P, bs + (size_t)k * BW_COUNT, I.bodies[b0 + k], k);
    int m = 0;
    for (int c = 0; c < nc; c++) {
        contact_rows<T, 0, APX>(S, stride, I, P, rows, jb, c0 + c, m, hinv);
        m += contact_rpc(I, P, c0 + c);
    }
    double resid = 0.0;
    if (m > 0) {
        for (int k = 0; k < nb; k++) body_tmp(S, stride, bs + (size_t)k * BW_COUNT, I.bodies[b0 + k], hinv);
        for (int i = 0; i < m; i++) row_setup<T, true, FB>(rows, jb, bs, i, hinv, P.sor_w);
        for (int it = 0; it < P.iters; it++) {
            const bool last = (it == P.iters - 1);
            const int *ord = I.order != nullptr ? I.order + (size_t)(it >> 3) * I.order_stride + r0 : nullptr;
            for (int i = 0; i < m; i++) {
                const T d = row_sor<T, APX>(rows, jb, bs, ord != nullptr ? ord[i] : i);
                if (last) resid += (double)d;
            }
        }
    }
    for (int k = 0; k < nb; k++) finish_body(S, bflags, stride, bs + (size_t)k * BW_COUNT, I.bodies[b0 + k], m > 0, h, I.damping);
    if (nc > 0) {
        atomicAdd(&diag->contacts, (unsigned long long)nc);
        atomicAdd(&diag->residual, resid);
    }
}

// ---- rows -> (lane, slot) of the wavefront that keeps them in registers --------------------------------------------------
// A lane has RPL slots of one row each.  Laid out plainly (row v in slot v / 64 of lane v % 64) the rows of one level sit in
// any slot, so every level step tests all RPL slots of every lane, and rows of one level that sit in different slots are
// updated one slot after the other.  Laid out BY LEVEL CLASS -- a row of level L in slot L mod RPL, lanes filled in row
// order -- a level step concerns one slot only: one test, one pass.  tab[c * 64 +
// t] = the row lane t holds in slot c (-1: none).  Returns false (and the plain layout) when a class has more than 64 rows.
// Called by the wavefront's 64 lanes; the caller synchronises before reading tab.
template <int RPL, class LevelOf>
__device__ __forceinline__ bool assign_row_slots(int nrow, int lane, short *tab, LevelOf level_of)
{
    int cnt[RPL];
#pragma unroll
    for (int c = 0; c < RPL; c++) { cnt[c] = 0; tab[c * 64 + lane] = (short)-1; }
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int base = 0; base < nrow; base += 64) {
        const int v = base + lane;
        const int cls = v < nrow ? level_of(v) % RPL : -1;
#pragma unroll
        for (int c = 0; c < RPL; c++) {
            const unsigned long long mk = __ballot(cls == c);
            if (cls == c) {
                const int rank = cnt[c] + __popcll(mk & lt);
                if (rank < 64) tab[c * 64 + rank] = (short)v;
            }
            cnt[c] += __popcll(mk);
        }
    }
    bool ok = true;
#pragma unroll
    for (int c = 0; c < RPL; c++) ok = ok && cnt[c] <= 64;
    if (!ok) {
#pragma unroll
        for (int c = 0; c < RPL; c++) { const int v = lane + 64 * c; tab[c * 64 + lane] = (short)(v < nrow ? v : -1); }
    }
    return ok;
}

// Pyramid rows (DMX_CONTACT_APPROX1) in the forms that keep a row in its owner's registers: the normal row of a contact and its
// friction rows share both bodies, so they sit on consecutive levels with a barrier between -- the normal row's owner leaves its
// multiplier in one LDS word (lamn[its row]) after every update, and a pyramid row's owner makes its bounds from that word before
// it updates its row: pyramid_bounds, row_sor's own spelling, then row_sor_lds as it is.  Per slot: fmu = RW_FMU of the row it holds,
// nrow = the row of the contact's normal.  Only the APX instantiations have one.
template <class T, int RPL> struct PyrSlots { T fmu[RPL]; int nrow[RPL]; T *lamn; };
template <class T, int RPL>
__device__ __forceinline__ void pyr_slot_load(PyrSlots<T, RPL> &p, int j, const T *rows, int r)
{
    p.fmu[j] = rows[(size_t)r * RW_COUNT + RW_FMU];
    p.nrow[j] = p.fmu[j] > T(0) ? r - (int)rows[(size_t)r * RW_COUNT + RW_FDIR] : r;
}
template <class T, int RPL, bool APX>
__device__ __forceinline__ T row_sor_slot(RowRegs<T> &r, T *fc, bool eager, const PyrSlots<T, RPL> *p, int j)
{
    if (APX) { if (p->fmu[j] > T(0)) pyramid_bounds(p->fmu[j], p->lamn[p->nrow[j]], r.lo, r.hi); }
    const T d = row_sor_lds<T, false>(nullptr, r, fc, eager);
    if (APX) { if (p->fmu[j] < T(0)) p->lamn[r.row] = r.lam; }
    return d;
}

// One sweep of the wavefront's rows.  classed: slot lv mod RPL holds every row of level lv (assign_row_slots).
template <class T, int RPL, bool LAST, bool APX = false>
__device__ __forceinline__ void wave_sweep(RowRegs<T> (&mine)[RPL], const int (&my_level)[RPL], int nlev, bool classed, T *fc_lds, bool eager,
                                           double &resid, const PyrSlots<T, RPL> *pyr = nullptr)
{
    if (classed) {
        for (int lv0 = 0; lv0 < nlev; lv0 += RPL) {
#pragma unroll
            for (int j = 0; j < RPL; j++) {
                if (lv0 + j < nlev) {
                    if (my_level[j] == lv0 + j) {
                        const T d = row_sor_slot<T, RPL, APX>(mine[j], fc_lds, eager, pyr, j);
                        if (LAST) resid += (double)d;
                    }
                    __syncthreads();
                }
            }
        }
    } else {
        for (int lv = 0; lv < nlev; lv++) {
#pragma unroll
            for (int j = 0; j < RPL; j++)
                if (my_level[j] == lv) {
                    const T d = row_sor_slot<T, RPL, APX>(mine[j], fc_lds, eager, pyr, j);
                    if (LAST) resid += (double)d;
                }
            __syncthreads();
        }
    }
}

// The sweeps of a small island by one wavefront (the first, if the launch has four): every row is OWNED by a lane and stays
// in that lane's registers, RPL rows per lane; a level step is "lanes whose row is in this level update it"; between two
// barriers only the bodies' accumulators in LDS are touched.  Returns the lane's share of the last sweep's residual.
template <class T, int RPL, bool APX = false>
__device__ __forceinline__ double wave_island_sweeps(T *rows, const int *jb, const int *row_level, int m, int nlev, int iters, int tid,
                                                     T *fc_lds, bool eager, T *lamn = nullptr)
{
    __shared__ short tab[RPL * 64];
    __shared__ int tab_classed;
    if (tid < 64) {
        const bool ok = RPL > 1 ? assign_row_slots<RPL>(m, tid, tab, [&](int v) { return row_level[v]; }) : false;
        if (RPL == 1) tab[tid] = (short)(tid < m ? tid : -1);
        if (tid == 0) tab_classed = ok ? 1 : 0;
    }
    __syncthreads();
    const bool classed = tab_classed != 0;
    RowRegs<T> mine[RPL];
    int my_level[RPL];
#pragma unroll
    for (int j = 0; j < RPL; j++) {
        const int r = tid < 64 ? (int)tab[j * 64 + tid] : -1;
        my_level[j] = -1;
        if (r >= 0) { row_load(rows, jb, r, mine[j]); my_level[j] = row_level[r]; }
    }
    __syncthreads();
    double resid = 0.0;
    if constexpr (APX) {
        PyrSlots<T, RPL> pyr;
        pyr.lamn = lamn;
#pragma unroll
        for (int j = 0; j < RPL; j++) {
            pyr.fmu[j] = T(0); pyr.nrow[j] = 0;
            if (my_level[j] >= 0) pyr_slot_load(pyr, j, rows, mine[j].row);
        }
        for (int it = 0; it + 1 < iters; it++) wave_sweep<T, RPL, false, true>(mine, my_level, nlev, classed, fc_lds, eager, resid, &pyr);
        if (iters > 0) wave_sweep<T, RPL, true, true>(mine, my_level, nlev, classed, fc_lds, eager, resid, &pyr);
    } else {
    for (int it = 0; it + 1 < iters; it++) wave_sweep<T, RPL, false>(mine, my_level, nlev, classed, fc_lds, eager, resid);
    if (iters > 0) wave_sweep<T, RPL, true>(mine, my_level, nlev, classed, fc_lds, eager, resid);      // the last sweep also sums its |delta lambda|
    }
#pragma unroll
    for (int j = 0; j < RPL; j++)
        if (my_level[j] >= 0) rows[(size_t)mine[j].row * RW_COUNT + RW_LAM] = mine[j].lam;
    return resid;
}

// ---- the same sweeps with a CONTACT (its normal and two friction rows) as the unit a lane owns -----------------------------
// The three rows of a contact are consecutive in creation order and share both bodies, so they sit on three consecutive levels
// and nothing else touches those bodies in between: a lane that owns all three fetches the two bodies' accumulators once,
// updates them in registers through the three rows, and writes them back once -- one LDS round trip per contact instead of
// per row, with exactly the row-by-row arithmetic.  Contact level = (level of its first row) / 3: two contacts sharing a body
// are at least three row levels apart, so they never get the same contact level and keep their order.  For islands whose
// contacts all carry the batch's surface with friction (three rows each).
template <class T> struct ContactRegs { T J[3][12], iMJ[3][12], rhs[3], ad[3], lo[3], hi[3], lam[3]; int l1, l2, row0; };

template <class T>
__device__ __forceinline__ void contact_load(const T *rows, const int *jb, int r0, ContactRegs<T> &c)
{
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const T *row = rows + (size_t)(r0 + d) * RW_COUNT;
#pragma unroll
        for (int j = 0; j < 12; j++) { c.J[d][j] = row[RW_J + j]; c.iMJ[d][j] = row[RW_IMJ + j]; }
        c.rhs[d] = row[RW_RHS]; c.ad[d] = row[RW_AD]; c.lo[d] = row[RW_LO]; c.hi[d] = row[RW_HI]; c.lam[d] = row[RW_LAM];
    }
    c.l1 = jb[2 * r0]; c.l2 = jb[2 * r0 + 1];
    c.row0 = r0;
}

// the same three rows made in registers, never stored: contact_rows + row_setup on thread-local arrays (the functions the
// other paths run on the row arrays in HBM, so the same bits), then straight into the lane's ContactRegs
template <class T>
__device__ __forceinline__ void contact_build(const T *S, int64_t stride, const IslandSet<T> &I, const StepParams<T> &P, const T *bs, int ci,
                                              T hinv, ContactRegs<T> &c)
{
    T lrows[3 * RW_COUNT];
    int ljb[6];
    contact_rows<T, 3>(S, stride, I, P, lrows, ljb, ci, 0, hinv);
#pragma unroll
    for (int d = 0; d < 3; d++) row_setup(lrows, ljb, bs, d, hinv, P.sor_w);
    contact_load(lrows, ljb, 0, c);
}

// FAST: the friction rows are unbounded (mu = inf, the reference's surface, main.c:687): their clamp -- two comparisons that are
// false and the selects behind them -- is left out; the normal row keeps its own.  Same values either way.
template <class T, bool LAST, bool FAST = false>
__device__ __forceinline__ void contact_sor_lds(ContactRegs<T> &c, T *fc, bool eager, double &resid)
{
    T *fc1 = fc + 6 * c.l1;
    T *fc2 = fc + 6 * (c.l2 >= 0 ? c.l2 : c.l1);
    const bool two = c.l2 >= 0;
    T a[6], b[6];
#pragma unroll
    for (int j = 0; j < 6; j++) a[j] = fc1[j];
    if (two || eager) {
#pragma unroll
        for (int j = 0; j < 6; j++) b[j] = fc2[j];
    } else {
#pragma unroll
        for (int j = 0; j < 6; j++) b[j] = T(0);
    }
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const T *J = c.J[d];
        const T old = c.lam[d];
        T delta = fma_(-old, c.ad[d], c.rhs[d]);
        delta -= fma_(a[5], J[5], fma_(a[4], J[4], fma_(a[3], J[3], fma_(a[2], J[2], fma_(a[1], J[1], a[0] * J[0])))));
        if (two)
            delta -= fma_(b[5], J[11], fma_(b[4], J[10], fma_(b[3], J[9], fma_(b[2], J[8], fma_(b[1], J[7], b[0] * J[6])))));
        const T nl = old + delta;
        if (FAST && d > 0) c.lam[d] = nl;
        else if (nl < c.lo[d]) { delta = c.lo[d] - old; c.lam[d] = c.lo[d]; }
        else if (nl > c.hi[d]) { delta = c.hi[d] - old; c.lam[d] = c.hi[d]; }
        else c.lam[d] = nl;
#pragma unroll
        for (int j = 0; j < 6; j++) a[j] = fma_(delta, c.iMJ[d][j], a[j]);
        if (two) {
#pragma unroll
            for (int j = 0; j < 6; j++) b[j] = fma_(delta, c.iMJ[d][6 + j], b[j]);
        }
        if (LAST) resid += (double)tabs(delta);
    }
#pragma unroll
    for (int j = 0; j < 6; j++) fc1[j] = a[j];
    if (two) {
#pragma unroll
        for (int j = 0; j < 6; j++) fc2[j] = b[j];
    }
}

// one sweep over the wavefront's contacts; slot cl mod CPL holds every contact of contact level cl when classed
template <class T, int CPL, bool LAST>
__device__ __forceinline__ void wave_contact_sweep(ContactRegs<T> (&mine)[CPL], const int (&my_cl)[CPL], int n_clev, bool classed, T *fc_lds,
                                                   bool eager, double &resid)
{
    if (classed) {
        for (int cl0 = 0; cl0 < n_clev; cl0 += CPL) {
#pragma unroll
            for (int j = 0; j < CPL; j++) {
                if (cl0 + j < n_clev) {
                    if (my_cl[j] == cl0 + j) contact_sor_lds<T, LAST>(mine[j], fc_lds, eager, resid);
                    __syncthreads();
                }
            }
        }
    } else {
        for (int cl = 0; cl < n_clev; cl++) {
#pragma unroll
            for (int j = 0; j < CPL; j++)
                if (my_cl[j] == cl) contact_sor_lds<T, LAST>(mine[j], fc_lds, eager, resid);
            __syncthreads();
        }
    }
}

// one island's sweeps with contacts as units (crow: the island's contacts' first rows, island-relative).  load(v, c): contact
// v's rows into c -- from the row arrays, or made on the spot (contact_build: then nothing is written back either).
template <class T, int CPL, class Load>
__device__ __forceinline__ double wave_island_contact_sweeps(T *rows, const int *row_level, const int *crow, int nc, int nlev,
                                                             int iters, int tid, T *fc_lds, bool eager, bool write_back, Load load)
{
    __shared__ short tab[CPL * 64];
    __shared__ int tab_classed;
    if (tid < 64) {
        const bool ok = CPL > 1 ? assign_row_slots<CPL>(nc, tid, tab, [&](int v) { return row_level[crow[v]] / 3; }) : false;
        if (CPL == 1) tab[tid] = (short)(tid < nc ? tid : -1);
        if (tid == 0) tab_classed = ok ? 1 : 0;
    }
    __syncthreads();
    const bool classed = tab_classed != 0;
    ContactRegs<T> mine[CPL];
    int my_cl[CPL];
#pragma unroll
    for (int j = 0; j < CPL; j++) {
        const int v = tid < 64 ? (int)tab[j * 64 + tid] : -1;
        my_cl[j] = -1;
        if (v >= 0) { load(v, mine[j]); mine[j].row0 = crow[v]; my_cl[j] = row_level[crow[v]] / 3; }
    }
    __syncthreads();
    const int n_clev = (nlev + 2) / 3;
    double resid = 0.0;
    for (int it = 0; it + 1 < iters; it++) wave_contact_sweep<T, CPL, false>(mine, my_cl, n_clev, classed, fc_lds, eager, resid);
    if (iters > 0) wave_contact_sweep<T, CPL, true>(mine, my_cl, n_clev, classed, fc_lds, eager, resid);
    if (write_back) {
#pragma unroll
        for (int j = 0; j < CPL; j++)
            if (my_cl[j] >= 0) {
#pragma unroll
                for (int d = 0; d < 3; d++) rows[(size_t)(mine[j].row0 + d) * RW_COUNT + RW_LAM] = mine[j].lam[d];
            }
    }
    return resid;
}

// rows a thread of the register-resident form holds at most: a workgroup of 256 owns up to 3 072 rows in f32, 1 536 in f64 (the
// reference's pen holds at most 512 bodies, body.h:6 -- their pile is 2 000-2 600 rows)
template <class T> constexpr int REGS_ROWS = sizeof(T) == 4 ? 3072 : 1536;      // rows a workgroup of the register form holds at most
template <class T, int WG> constexpr int REGS_ROWS_PER_THREAD = REGS_ROWS<T> / WG;

// The sweeps of a large island by a whole workgroup with every row in REGISTERS: the row at position t of the island's level
// lists (rows grouped by level, lev_rows) belongs to thread t mod WG, RPL rows per thread, for all twenty sweeps; a level step is
// "threads holding a row of this level update it" and an LDS hand-over of the accumulators.  Nothing is fetched from device
// memory between the first sweep and the last.  (Streaming a lane's row of each level from L2 instead -- solve_island_wg's
// general form -- makes every level step one L2 round trip long: 0.9 us in the reference's pen, 45 levels x 20 sweeps.)  A level's
// rows are consecutive positions, so they sit in at most two of a thread's slots (one, if the level is no wider than what is
// left of the slot): a wavefront runs one or two row updates per level, not RPL.  Returns the thread's share of the last sweep's residual.
template <class T, int RPL, int WG, bool APX = false>
__device__ __forceinline__ double wg_island_sweeps(T *rows, const int *jb, const int *row_level, const int *lev_rows, int m, int nlev, int iters,
                                                   int tid, T *fc_lds, T *lamn = nullptr)
{
    RowRegs<T> mine[RPL];
    int my_level[RPL];
#pragma unroll
    for (int j = 0; j < RPL; j++) {
        const int t = tid + WG * j;
        my_level[j] = -1;
        if (t < m) { const int r = lev_rows[t]; row_load(rows, jb, r, mine[j]); my_level[j] = row_level[r]; }
    }
    double resid = 0.0;
    PyrSlots<T, APX ? RPL : 1> pyr;
    if constexpr (APX) {
        pyr.lamn = lamn;
#pragma unroll
        for (int j = 0; j < RPL; j++) {
            pyr.fmu[j] = T(0); pyr.nrow[j] = 0;
            if (my_level[j] >= 0) pyr_slot_load(pyr, j, rows, mine[j].row);
        }
    }
    for (int it = 0; it < iters; it++) {
        const bool last = it + 1 == iters;
        for (int lv = 0; lv < nlev; lv++) {
#pragma unroll
            for (int j = 0; j < RPL; j++)
                if (my_level[j] == lv) {
                    T d;
                    if constexpr (APX) d = row_sor_slot<T, RPL, true>(mine[j], fc_lds, true, &pyr, j);
                    else d = row_sor_lds<T, false>(nullptr, mine[j], fc_lds, true);
                    if (last) resid += (double)d;
                }
            lds_barrier();
        }
    }
#pragma unroll
    for (int j = 0; j < RPL; j++)
        if (my_level[j] >= 0) rows[(size_t)mine[j].row * RW_COUNT + RW_LAM] = mine[j].lam;
    return resid;
}

// The same with CONTACTS as units (three rows per contact throughout): the u-th contact in level order belongs to thread u mod WG,
// CPL contacts a thread.  A contact's normal and two friction rows sit on consecutive levels on the same two bodies, so a lane that
// holds all three fetches the bodies' accumulators once, carries them through the three row updates in registers and writes them
// back once: one LDS round trip and one barrier per CONTACT level where the row form pays three (the pen's pile: 150 row levels x
// 20 sweeps, each ~260 cycles of which ~130 are the round trip and the barrier).  The arithmetic per row is row_sor_lds's, in the
// same order: same bits.  cfirst: nc ints of LDS scratch.
template <class T, int CPL, int WG>
__device__ __forceinline__ double wg_island_contact_sweeps(T *rows, const int *jb, const int *row_level, const int *lev_rows, const int *lev_off,
                                                           int m, int nlev, int iters, int tid, T *fc_lds, int *cfirst)
{
    const int nc = m / 3, n_clev = nlev / 3;
    // contacts in level order: the rows of level 3 cl are the first rows of contact level cl's contacts, and the levels below hold
    // exactly three rows of every earlier contact
    for (int p = tid; p < m; p += WG) {
        const int r = lev_rows[p], lv = row_level[r];
        if (lv % 3 == 0) { const int a = lev_off[lv] - lev_off[0]; cfirst[a / 3 + (p - a)] = r; }
    }
    __syncthreads();
    ContactRegs<T> mine[CPL];
    int my_cl[CPL];
#pragma unroll
    for (int j = 0; j < CPL; j++) {
        const int u = tid + WG * j;
        my_cl[j] = -1;
        if (u < nc) { const int r0 = cfirst[u]; contact_load(rows, jb, r0, mine[j]); my_cl[j] = row_level[r0] / 3; }
    }
    double resid = 0.0;
    // (do this island's friction rows ever clamp?  Asked of the rows themselves: the bounds sit in the registers just loaded)
    int unbounded = 1;
#pragma unroll
    for (int j = 0; j < CPL; j++)
        if (my_cl[j] >= 0)
            unbounded &= (mine[j].lo[1] == -Limits<T>::inf() && mine[j].hi[1] == Limits<T>::inf() && mine[j].lo[2] == -Limits<T>::inf() &&
                          mine[j].hi[2] == Limits<T>::inf()) ? 1 : 0;
    const bool fast = __syncthreads_and(unbounded) != 0;
    auto sweeps = [&](auto FASTT) {
        constexpr bool F = decltype(FASTT)::value;
        for (int it = 0; it + 1 < iters; it++)
            for (int cl = 0; cl < n_clev; cl++) {
#pragma unroll
                for (int j = 0; j < CPL; j++)
                    if (my_cl[j] == cl) contact_sor_lds<T, false, F>(mine[j], fc_lds, true, resid);
                lds_barrier();
            }
        if (iters > 0)
            for (int cl = 0; cl < n_clev; cl++) {
#pragma unroll
                for (int j = 0; j < CPL; j++)
                    if (my_cl[j] == cl) contact_sor_lds<T, true, F>(mine[j], fc_lds, true, resid);
                lds_barrier();
            }
    };
    if (fast) sweeps(std::true_type{}); else sweeps(std::false_type{});
#pragma unroll
    for (int j = 0; j < CPL; j++)
        if (my_cl[j] >= 0) {
#pragma unroll
            for (int d = 0; d < 3; d++) rows[(size_t)(mine[j].row0 + d) * RW_COUNT + RW_LAM] = mine[j].lam[d];
        }
    return resid;
}

// ================================================================================ one workgroup per large island
constexpr int FC_LDS_BYTES = 48 * 1024;     // islands of up to 2048 (f32) / 1024 (f64) bodies keep their accumulators in LDS
// (WAVE_ISLAND_ROWS, dmx_internal.hpp: islands of up to that many rows are solved by one wavefront with the rows in registers;
//  such an island has at most 2 x 256 bodies, which always fit the LDS above)

// REGS: islands of up to WG x 12 (f32) / WG x 6 (f64) rows keep them in registers for the sweeps (wg_island_sweeps); a separate
// instantiation, so that the streaming forms keep their register budget
// APX: see solve_islands_body.  Islands of such a tick take the row-unit forms (a lane that owns a whole contact would need the
// markers in its ContactRegs, which are close to the register budget as they are), and those too large for a workgroup's registers
// the form that sweeps the row table itself (row_sor), where the normal row's multiplier is simply there.
template <class T, int WG, bool REGS, bool FB = false, bool APX = false>
__device__ __forceinline__ void solve_island_wg_body(T *__restrict__ S, const uint8_t *__restrict__ bflags,
                                                     int64_t stride, const IslandSet<T> &I, const StepParams<T> &P,
                                                     StepDiag *__restrict__ diag, int lds_bodies, const ExactCounts *__restrict__ dc,
                                                     int sched_ints, unsigned bidx, unsigned nblocks)
{
    // dc: a launch enqueued before the host has seen the tick's counts (careful_tick, small scenes) -- the grid covers the
    // capacity, the record on the device says how many islands there are and whether this launch may act at all
    if (dc != nullptr && (dc->spec_ok == 0u || bidx >= dc->nbig)) return;
    const int isl = I.big_list[bidx];
    const int tid = threadIdx.x;
    const T h = P.h, hinv = T(1) / h;
    const int b0 = I.body_off[isl], nb = I.body_off[isl + 1] - b0;
    const int c0 = I.con_off[isl], nc = I.con_off[isl + 1] - c0;
    const int r0 = I.row_off[isl];
    T *bs = I.bscr + (size_t)b0 * BW_COUNT;
    T *rows = I.rows + (size_t)r0 * RW_COUNT;
    int *jb = I.rowjb + 2 * (size_t)r0;
    const int lv0 = I.big[isl];                               // this island's slice of the level schedule
    const int nlev = I.lev_count[bidx];
    const int *lev_off = I.lev_off + lv0;                     // [nlev+1], offsets into lev_rows (island-relative rows)
    const int m = lev_off[nlev] - lev_off[0];

    // Small island, three rows per contact throughout (the batch's surface with friction, or per-contact surfaces that all
    // have it): one wavefront, a lane owns a contact and makes its rows in its own registers -- they never go to HBM.
    const bool wave = nb <= lds_bodies && nlev > 0 && m <= WAVE_ISLAND_ROWS;         // (workgroup-uniform, like all of this)
    bool by_contact = false;
    if (wave) {
        by_contact = I.cmu == nullptr && P.mu > 0;
        if (I.cmu != nullptr) {
            int all3 = 1;
            for (int c = tid; c < nc; c += WG) all3 &= I.cmu[c0 + c] > 0 ? 1 : 0;
            by_contact = __syncthreads_and(all3) != 0;
        }
        by_contact = by_contact && (nc <= 64 || sizeof(T) == 4);      // (a contact's rows are 90 reals of registers: two per lane in f32)
        by_contact = by_contact && !FB;                              // (feedback reads the row table: the rows are built there, by the row form)
        by_contact = by_contact && !APX;
    }
    T *lamn = nullptr;                                               // one word per row for the normal rows' multipliers (PyrSlots)
    if constexpr (APX) {
        __shared__ T lamn_s[REGS ? REGS_ROWS<T> : WAVE_ISLAND_ROWS];
        lamn = lamn_s;
    }

    for (int k = tid; k < nb; k += WG) stage_body(S, bflags, stride, I, P, bs + (size_t)k * BW_COUNT, I.bodies[b0 + k], k);
    __syncthreads();
    if (!by_contact)
        for (int c = tid; c < nc; c += WG) contact_rows<T, 0, APX>(S, stride, I, P, rows, jb, c0 + c, I.crow[c0 + c], hinv);
    for (int k = tid; k < nb; k += WG) body_tmp(S, stride, bs + (size_t)k * BW_COUNT, I.bodies[b0 + k], hinv);
    __syncthreads();
    if (!by_contact) {
        for (int i = tid; i < m; i += WG) row_setup<T, true, FB>(rows, jb, bs, i, hinv, P.sor_w);
        __syncthreads();
    }

    double resid = 0.0;
    // LDS staging: the only data one level hands to the next is the bodies' constraint-force accumulators (6 reals per
    // body); they live in LDS for the sweeps.  A row's own data does not depend on other rows, so each lane fetches its
    // row of the NEXT level before it works on this one: between two barriers only LDS traffic and arithmetic remain.
    // dynamic LDS, sized by the launch for the largest island in it (small islands must not reserve 48 KB each: that
    // would cap a CU at three of them)
    extern __shared__ __align__(16) unsigned char fc_raw[];
    T *fc_lds = reinterpret_cast<T *>(fc_raw);
    const bool use_lds = nb <= lds_bodies && nlev > 0;    // workgroup-uniform
    if (use_lds && m <= WAVE_ISLAND_ROWS) {
        // Small island, one wavefront (the first, if the launch has four): every row is OWNED by a lane for the whole solve
        // (row r by lane r mod 64) and stays in that lane's registers; a level step is "lanes whose row is in this level
        // update it".  Nothing is fetched between two barriers but the bodies' accumulators in LDS.  Only row_level is read
        // of the schedule: the device-side builder (dmx_exact.hip) leaves the per-level row lists of such islands unbuilt.
        for (int k = tid; k < nb; k += WG)
            for (int j = 0; j < 6; j++) fc_lds[6 * k + j] = bs[(size_t)k * BW_COUNT + BW_FC + j];
        const int *row_level = I.row_level + lev_off[0];
        // (rows per lane as a template parameter: an island of up to 64 rows pays for one row's tests per level, not four)
        const bool eager = (dc != nullptr ? dc->nbig : nblocks) < 2048u;           // few islands: every one waits on its own chain of rows
        auto build = [&](int v, ContactRegs<T> &c) { contact_build(S, stride, I, P, bs, c0 + v, hinv, c); };
        if (by_contact && nc <= 64) resid = wave_island_contact_sweeps<T, 1>(rows, row_level, I.crow + c0, nc, nlev, P.iters, tid, fc_lds, eager, false, build);
        else if (by_contact) resid = wave_island_contact_sweeps<T, sizeof(T) == 4 ? 2 : 1>(rows, row_level, I.crow + c0, nc, nlev, P.iters, tid, fc_lds, eager, false, build);
        else if (m <= 64) resid = wave_island_sweeps<T, 1, APX>(rows, jb, row_level, m, nlev, P.iters, tid, fc_lds, eager, lamn);
        else if (m <= 128) resid = wave_island_sweeps<T, 2, APX>(rows, jb, row_level, m, nlev, P.iters, tid, fc_lds, eager, lamn);
        else resid = wave_island_sweeps<T, WAVE_ISLAND_ROWS / 64, APX>(rows, jb, row_level, m, nlev, P.iters, tid, fc_lds, eager, lamn);
        for (int k = tid; k < nb; k += WG)
            for (int j = 0; j < 6; j++) bs[(size_t)k * BW_COUNT + BW_FC + j] = fc_lds[6 * k + j];
    } else if (REGS && use_lds && m <= REGS_ROWS<T>) {
        const int contact_scratch_ints = sched_ints;          // (REGS launches: room behind the accumulators for one int per contact)
        for (int k = tid; k < nb; k += WG)
            for (int j = 0; j < 6; j++) fc_lds[6 * k + j] = bs[(size_t)k * BW_COUNT + BW_FC + j];
        __syncthreads();
        const int *row_level = I.row_level + lev_off[0], *lev_rows = I.lev_rows + lev_off[0];
        // (rows per thread as a template parameter: 32 registers a row in f32, 64 in f64 -- of a lane's 512 at one wave per SIMD)
        constexpr int RMAX = REGS_ROWS_PER_THREAD<T, WG>;          // 6 (f32) / 3 (f64) at 512 threads, 12 / 6 at 256
        // three rows per contact throughout (the batch's surface with friction, or per-contact surfaces that all have it) and at
        // most two contacts a thread (a contact is 90 registers in f32): contacts as units
        bool all3 = !APX && sizeof(T) == 4 && m == 3 * nc && nlev % 3 == 0 && nc <= 2 * WG && contact_scratch_ints >= nc && (I.cmu != nullptr || P.mu > 0);
        if (all3 && I.cmu != nullptr) {
            int a3 = 1;
            for (int c = tid; c < nc; c += WG) a3 &= I.cmu[c0 + c] > 0 ? 1 : 0;
            all3 = __syncthreads_and(a3) != 0;
        }
        int *cfirst = reinterpret_cast<int *>(fc_lds + (size_t)6 * lds_bodies);
        if (all3 && nc <= WG) resid = wg_island_contact_sweeps<T, 1, WG>(rows, jb, row_level, lev_rows, lev_off, m, nlev, P.iters, tid, fc_lds, cfirst);
        else if (all3) resid = wg_island_contact_sweeps<T, sizeof(T) == 4 ? 2 : 1, WG>(rows, jb, row_level, lev_rows, lev_off, m, nlev, P.iters, tid, fc_lds, cfirst);
        else if (m <= 2 * WG) resid = wg_island_sweeps<T, 2, WG, APX>(rows, jb, row_level, lev_rows, m, nlev, P.iters, tid, fc_lds, lamn);
        else if (m <= 3 * WG || RMAX <= 3) resid = wg_island_sweeps<T, RMAX < 3 ? RMAX : 3, WG, APX>(rows, jb, row_level, lev_rows, m, nlev, P.iters, tid, fc_lds, lamn);
        else if (m <= 4 * WG || RMAX <= 4) resid = wg_island_sweeps<T, RMAX < 4 ? RMAX : 4, WG, APX>(rows, jb, row_level, lev_rows, m, nlev, P.iters, tid, fc_lds, lamn);
        else if (m <= 6 * WG || RMAX <= 6) resid = wg_island_sweeps<T, RMAX < 6 ? RMAX : 6, WG, APX>(rows, jb, row_level, lev_rows, m, nlev, P.iters, tid, fc_lds, lamn);
        else if (m <= 8 * WG || RMAX <= 8) resid = wg_island_sweeps<T, RMAX < 8 ? RMAX : 8, WG, APX>(rows, jb, row_level, lev_rows, m, nlev, P.iters, tid, fc_lds, lamn);
        else resid = wg_island_sweeps<T, RMAX, WG, APX>(rows, jb, row_level, lev_rows, m, nlev, P.iters, tid, fc_lds, lamn);
        __syncthreads();
        for (int k = tid; k < nb; k += WG)
            for (int j = 0; j < 6; j++) bs[(size_t)k * BW_COUNT + BW_FC + j] = fc_lds[6 * k + j];
    } else if (use_lds && !APX) {
        for (int k = tid; k < nb; k += WG)
            for (int j = 0; j < 6; j++) fc_lds[6 * k + j] = bs[(size_t)k * BW_COUNT + BW_FC + j];
        // The schedule itself in LDS when the launch made room for it (sched_ints): a level step's row is found by two dependent
        // look-ups (the level's offset, then the row list) before the row can be fetched -- three L2 round trips in a chain, the
        // whole length of a level step, when they go to device memory; here they are LDS reads and the fetch is issued two
        // steps ahead of its use.
        int *loff = reinterpret_cast<int *>(fc_lds + (size_t)6 * lds_bodies), *lrows = loff + nlev + 1;
        const bool sched = sched_ints >= nlev + 1 + m;
        if (sched) {
            for (int q = tid; q <= nlev; q += WG) loff[q] = lev_off[q] - lev_off[0];
            for (int t = tid; t < m; t += WG) lrows[t] = I.lev_rows[lev_off[0] + t];
        }
        __syncthreads();
        const int total = nlev * P.iters;
        auto first_row = [&](int lv) {
            if (sched) { const int t = loff[lv] + tid; return t < loff[lv + 1] ? lrows[t] : -1; }
            const int t = lev_off[lv] + tid;
            return t < lev_off[lv + 1] ? I.lev_rows[t] : -1;
        };
        auto next_level = [&](int lv) { return lv + 1 == nlev ? 0 : lv + 1; };
        // rows of steps g, g + 1, g + 2 (a lane's row of each level: position tid of the level's list)
        RowRegs<T> cur, n1, n2;
        int lv0 = 0, lv1 = next_level(0), lv2 = next_level(lv1);
        int rc = total > 0 ? first_row(lv0) : -1, r1 = total > 1 ? first_row(lv1) : -1, r2 = -1;
        if (rc >= 0) row_load(rows, jb, rc, cur);
        if (r1 >= 0) row_load(rows, jb, r1, n1);
        for (int g = 0; g < total; g++) {
            const bool last = g >= total - nlev;
            r2 = g + 2 < total ? first_row(lv2) : -1;
            if (r2 >= 0) row_load(rows, jb, r2, n2);
            if (rc >= 0) {
                const T d = row_sor_lds(rows, cur, fc_lds);
                if (last) resid += (double)d;
                // schedules of one or two levels: a fetch issued before this update holds the old multiplier
                if (r1 == rc) n1.lam = cur.lam;
                if (r2 == rc) n2.lam = cur.lam;
            }
            {                                                                       // levels wider than the workgroup
                const int a = sched ? loff[lv0] + lev_off[0] : lev_off[lv0], e = sched ? loff[lv0 + 1] + lev_off[0] : lev_off[lv0 + 1];
                for (int t = a + tid + WG; t < e; t += WG) {
                    RowRegs<T> x;
                    row_load(rows, jb, I.lev_rows[t], x);
                    const T d = row_sor_lds(rows, x, fc_lds);
                    if (last) resid += (double)d;
                }
            }
            // the next level reads the accumulators this one wrote: an LDS hand-over.  NOT __syncthreads(): that also waits for
            // every outstanding global access (vmcnt(0)) -- the rows fetched for the levels ahead, which are in flight precisely
            // so that nobody waits for them; with it every level step was one L2 round trip long (800 ns in the pen's pile).
            lds_barrier();
            cur = n1; rc = r1; n1 = n2; r1 = r2;
            lv0 = lv1; lv1 = lv2; lv2 = next_level(lv2);
        }
        for (int k = tid; k < nb; k += WG)                     // back for finish_body (same lane, same bodies)
            for (int j = 0; j < 6; j++) bs[(size_t)k * BW_COUNT + BW_FC + j] = fc_lds[6 * k + j];
    } else {
        for (int it = 0; it < P.iters; it++) {
            const bool last = (it == P.iters - 1);
            for (int lv = 0; lv < nlev; lv++) {
                const int a = lev_off[lv], e = lev_off[lv + 1];
                for (int t = a + tid; t < e; t += WG) {
                    const T d = row_sor<T, APX>(rows, jb, bs, I.lev_rows[t]);
                    if (last) resid += (double)d;
                }
                __syncthreads();                              // the next level reads the fc this one wrote
            }
        }
    }
    for (int k = tid; k < nb; k += WG) finish_body(S, bflags, stride, bs + (size_t)k * BW_COUNT, I.bodies[b0 + k], m > 0, h, I.damping);

    // residual: wave reduction, then one atomic per wave
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) resid += __shfl_xor(resid, o, 64);
    if ((tid & 63) == 0) atomicAdd(&diag->residual, resid);
    if (tid == 0) atomicAdd(&diag->contacts, (unsigned long long)nc);
}

}  // namespace dmx
