// dmx_small.hip -- one tick of a small world in one launch.
//
// dmxBatchStepJoints on a world of tens of bodies is launch- and copy-bound on the general path (two staging copies, a fill,
// up to four kernels one behind the other, a pack kernel and a copy back at the next pose read).  small_world_tick does the
// tick's device work in one grid:
//   workgroups [0, n_big)   one island with rows each: QuickStep's sweeps (solve_island_wg_body, the one-wavefront form) or
//                           dWorldStep's LDS solve (lcp_island_lds_body) -- the functions the general path's kernels wrap;
//   workgroups behind them  a lane per island: free bodies (solve_islands_body) and, for QuickStep, one-body islands of 1..8
//                           contacts (solve_singles_body / solve_singles_lds_body).
// The island tables and contact reals are read through the device address of the host's pinned staging; every stepped body's
// 13 state reals go to the slab as always and to a host-mapped mirror that dmxBatchDownload(DMX_STATE) serves from.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "dmx_islands_dev.hpp"
#include "dmx_lcp_lds.hpp"
#include "dmx_small.hpp"
#include "dmx_autodisable.hpp"

namespace dmx {

template <class T> __device__ __forceinline__ void mirror_body(const T *S, T *mirror, int s)
{
#pragma unroll
    for (int c = 0; c < C_MASS; c++) mirror[(size_t)C_MASS * s + c] = S[slab_ix(c, s)];
}

// feedback of island isl's entries first + k step, k = 0, 1, ...: the joints whose first entry they are (joint_feedback,
// dmx_island_rows.hpp) -> F.fb, which is host-mapped here.  Called behind the island's solve, by the threads that ran it.
template <class T> __device__ __forceinline__ void island_feedback(const IslandSet<T> &I, const StepParams<T> &P, const FeedbackSet<T> &F, int isl, int first, int step)
{
    const int c0 = I.con_off[isl], c1 = I.con_off[isl + 1];
    const T *rows = I.rows + (size_t)I.row_off[isl] * RW_COUNT;
    for (int d = c0 + first; d < c1; d += step) {
        const int o = F.out[d];
        if (o < 0) continue;
        T out[12];
        joint_feedback(I, P, rows, d, F.info[d], F.mode == FB_SCALED, out);
        for (int j = 0; j < 12; j++) F.fb[(size_t)12 * o + j] = out[j];
    }
}

// FB: a tick made with feedback on -- an instantiation of its own, so that the others are the kernels they were before feedback
// existed (F is an argument they never read).
// APX: a QuickStep tick with pyramid rows (DMX_CONTACT_APPROX1): the island functions' APX instantiations, made with FB's store on --
// F.mode says whether the tick reports feedback too.  (Under dWorldStep such a tick takes the general path.)
// AD: a tick that stepped a body with DMX_BODY_AUTODISABLE, or left an asleep island out: the thread that finished a body applies
// the end-of-tick rule (idle_update) before it mirrors the body, and writes the body's flag byte to the host-mapped flag mirror.
// An instantiation of its own again: a tick without such a body launches the kernel it launched before auto-disable existed.
template <class T, bool EXACT, bool FB = false, bool APX = false, bool AD = false>
__global__ __launch_bounds__(EXACT ? 256 : 64) void small_world_tick(T *S, const uint8_t *bflags, int64_t stride, IslandSet<T> I, StepParams<T> P,
                                                                     StepDiag *diag, SmallTick<T> K, FeedbackSet<T> F)
{
    constexpr int WG = EXACT ? 256 : 64;
    const int tid = threadIdx.x;
    if (blockIdx.x == 0 && tid == 0) { K.diag_next->contacts = 0ull; K.diag_next->residual = 0.0; }
    if (blockIdx.x < (unsigned)I.n_big) {
        if (EXACT) lcp_island_lds_body<T, WG>(S, bflags, stride, I, P, diag, K.murty, K.tol_rel, blockIdx.x);
        else solve_island_wg_body<T, WG, false, FB, APX>(S, bflags, stride, I, P, diag, K.lds_bodies, (const ExactCounts *)nullptr, 0, blockIdx.x, (unsigned)I.n_big);
        __syncthreads();
        const int isl = I.big_list[blockIdx.x];
        if (FB && (!APX || F.mode != FB_OFF)) island_feedback(I, P, F, isl, tid, WG);                                       // (the rows' lambda is behind the barrier)
        const int b0 = I.body_off[isl], nb = I.body_off[isl + 1] - b0;
        for (int k = tid; k < nb; k += WG) {                                                // (body k was finished by this thread)
            const int s = I.bodies[b0 + k];
            if (AD) K.ad_mirror[s] = idle_update<T>(S, K.ad_flags, K.ad_steps, K.ad_time, K.ad, s);
            mirror_body(S, K.mirror, s);
        }
    } else {
        constexpr int LANES = EXACT ? WG : SMALL_TAIL_LANES;
        const int isl = (int)(blockIdx.x - (unsigned)I.n_big) * LANES + tid;
        if (tid < LANES && isl < I.n_islands && I.big[isl] < 0) {
            solve_islands_body<T, FB, APX>(S, bflags, stride, I, P, diag, isl);        // (each of the three takes its own kind of island)
            if (!EXACT && !FB) {                  // (feedback on: the row form above has taken them, I.singles = 0)
                solve_singles_body<T>(S, bflags, stride, I, P, diag, isl);
                solve_singles_lds_body<T>(S, bflags, stride, I, P, diag, isl, LANES, tid);
            }
            if (FB && (!APX || F.mode != FB_OFF)) island_feedback(I, P, F, isl, 0, 1);
            const int b0 = I.body_off[isl], nb = I.body_off[isl + 1] - b0;
            for (int k = 0; k < nb; k++) {
                const int s = I.bodies[b0 + k];
                if (AD) K.ad_mirror[s] = idle_update<T>(S, K.ad_flags, K.ad_steps, K.ad_time, K.ad, s);
                mirror_body(S, K.mirror, s);
            }
        }
    }
    if (K.full)         // slots outside every island (not alive): nobody else brings the mirror up to date for them
        for (int s = (int)(blockIdx.x * WG) + tid; s < K.n_slots; s += (int)(gridDim.x * WG)) {
            // AD: ... nor for the slots of the asleep islands this tick left out, which the host marked in the flag mirror
            // (SMALL_AD_SKIPPED: no thread of this tick writes such a slot's entry, so reading it here races with nobody)
            if (AD ? (!(K.ad_flags[s] & BF_ALIVE) || (K.ad_mirror[s] & SMALL_AD_SKIPPED)) : !(bflags[s] & BF_ALIVE)) mirror_body(S, K.mirror, s);
        }
}

size_t small_tick_sor_lds(int real_bytes, int max_bodies, int *lds_bodies)
{
    const int lds_cap = FC_LDS_BYTES / (6 * real_bytes);
    *lds_bodies = std::min(std::max(max_bodies, 1), lds_cap);
    const size_t wg = (size_t)*lds_bodies * 6 * real_bytes;
    const size_t tail = (size_t)SMALL_TAIL_LANES * 3 * SINGLE_MAXC_LDS * RS_FIELDS * real_bytes;
    return std::max(wg, tail);
}

template <class T, bool FB, bool APX = false, bool AD = false>
static hipError_t launch_small_tick_fb(T *S, const uint8_t *bflags, int64_t stride, const IslandSet<T> &I, const StepParams<T> &P, StepDiag *diag,
                                       const SmallTick<T> &K, const FeedbackSet<T> &F, bool exact, size_t lds_bytes, hipStream_t st)
{
    // (always at least one workgroup: an empty world's tick still rotates the diagnostics slots and may fill the mirror)
    const int lanes = exact ? 256 : SMALL_TAIL_LANES;
    const unsigned grid = (unsigned)I.n_big + (unsigned)std::max(1, (I.n_islands + lanes - 1) / lanes);
    if (exact && !APX) {
        if (lds_bytes > (size_t)64 * 1024) {
            const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void *>(&small_world_tick<T, true, FB, false, AD>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
            if (ea != hipSuccess) return ea;
        }
        hipLaunchKernelGGL((small_world_tick<T, true, FB, false, AD>), dim3(grid), dim3(256), lds_bytes, st, S, bflags, stride, I, P, diag, K, F);
    } else {
        hipLaunchKernelGGL((small_world_tick<T, false, FB, APX, AD>), dim3(grid), dim3(64), lds_bytes, st, S, bflags, stride, I, P, diag, K, F);
    }
    return hipGetLastError();
}
template <class T>
hipError_t launch_small_tick(T *S, const uint8_t *bflags, int64_t stride, const IslandSet<T> &I, const StepParams<T> &P, StepDiag *diag,
                             const SmallTick<T> &K, const FeedbackSet<T> &F, bool exact, size_t lds_bytes, hipStream_t st, bool pyramid, bool ad)
{
    if (ad) {
        if (pyramid) return exact ? hipErrorInvalidValue : launch_small_tick_fb<T, true, true, true>(S, bflags, stride, I, P, diag, K, F, false, lds_bytes, st);
        return F.mode != FB_OFF ? launch_small_tick_fb<T, true, false, true>(S, bflags, stride, I, P, diag, K, F, exact, lds_bytes, st)
                                : launch_small_tick_fb<T, false, false, true>(S, bflags, stride, I, P, diag, K, F, exact, lds_bytes, st);
    }
    if (pyramid) return exact ? hipErrorInvalidValue : launch_small_tick_fb<T, true, true>(S, bflags, stride, I, P, diag, K, F, false, lds_bytes, st);
    return F.mode != FB_OFF ? launch_small_tick_fb<T, true>(S, bflags, stride, I, P, diag, K, F, exact, lds_bytes, st)
                            : launch_small_tick_fb<T, false>(S, bflags, stride, I, P, diag, K, F, exact, lds_bytes, st);
}
template hipError_t launch_small_tick<float>(float *, const uint8_t *, int64_t, const IslandSet<float> &, const StepParams<float> &, StepDiag *,
                                             const SmallTick<float> &, const FeedbackSet<float> &, bool, size_t, hipStream_t, bool, bool);
template hipError_t launch_small_tick<double>(double *, const uint8_t *, int64_t, const IslandSet<double> &, const StepParams<double> &, StepDiag *,
                                              const SmallTick<double> &, const FeedbackSet<double> &, bool, size_t, hipStream_t, bool, bool);

hipError_t dmx_touch_small(int real_bytes)
{
    hipFuncAttributes a;
    hipError_t e = hipSuccess;
    auto touch = [&](const void *k) { const hipError_t r = hipFuncGetAttributes(&a, k); if (r != hipSuccess) e = r; };
    if (real_bytes == 4) { touch((const void *)&small_world_tick<float, false>); touch((const void *)&small_world_tick<float, true>); }
    else { touch((const void *)&small_world_tick<double, false>); touch((const void *)&small_world_tick<double, true>); }
    return e;
}

}  // namespace dmx
