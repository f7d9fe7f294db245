// dmx_islands.hip -- general dynamics-island step: dWorldQuickStep over islands of any size, fed by an
// explicit contact list (the contact joints of dJointCreateContact + dJointAttach,
// /root/reference/src/main.c:690-691, or the device narrowphase's output).
//
// The SOR sweep is a sequential Gauss-Seidel over the island's rows in creation order.  Two kernels run the
// same per-body / per-contact / per-row phase functions and therefore give the same bits:
//   solve_islands    -- one lane per island: plenty of small islands in flight at once;
//   solve_island_wg  -- one workgroup per LARGE island (a pile): every phase is spread over the workgroup's lanes;
//                       the sweep follows a level schedule (row r's level = 1 + the latest level of an earlier row
//                       sharing a body with r): rows of one level touch disjoint bodies, so updating them
//                       concurrently gives exactly the sequential result; one barrier per level.
// Rows and per-body scratch live in HBM/L2; solve_island_wg keeps the constraint-force accumulators in LDS during the
// sweeps and prefetches each lane's next row across the level barrier.  Single bodies resting on the ground plane never come here: they take
// the fused register-resident path (step_plane).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include "dmx_internal.hpp"
#include "dmx_exact.hpp"
#include "dmx_math.hpp"
#include "dmx_step_fused.hpp"

#include "dmx_island_rows.hpp"
#include "dmx_islands_dev.hpp"

namespace dmx {


// the kernels' bodies: dmx_islands_dev.hpp
template <class T>
__global__ __launch_bounds__(64) void solve_singles(T *__restrict__ S, const uint8_t *__restrict__ bflags, int64_t stride,
                                                    IslandSet<T> I, StepParams<T> P, StepDiag *__restrict__ diag)
{
    solve_singles_body<T>(S, bflags, stride, I, P, diag, (int)(blockIdx.x * blockDim.x + threadIdx.x));
}
template <class T>
__global__ __launch_bounds__(64) void solve_singles_lds(T *__restrict__ S, const uint8_t *__restrict__ bflags, int64_t stride,
                                                        IslandSet<T> I, StepParams<T> P, StepDiag *__restrict__ diag)
{
    const int lanes = blockDim.x, lane = threadIdx.x;
    solve_singles_lds_body<T>(S, bflags, stride, I, P, diag, (int)(blockIdx.x * lanes + lane), lanes, lane);
}
template <class T, bool FB = false, bool APX = false>
__global__ __launch_bounds__(64) void solve_islands(T *__restrict__ S, const uint8_t *__restrict__ bflags,
                                                    int64_t stride, IslandSet<T> I, StepParams<T> P,
                                                    StepDiag *__restrict__ diag)
{
    solve_islands_body<T, FB, APX>(S, bflags, stride, I, P, diag, (int)(blockIdx.x * blockDim.x + threadIdx.x));
}
template <class T, int WG, bool REGS = false, bool FB = false, bool APX = false>
__global__ __launch_bounds__(WG) void solve_island_wg(T *__restrict__ S, const uint8_t *__restrict__ bflags,
                                                      int64_t stride, IslandSet<T> I, StepParams<T> P,
                                                      StepDiag *__restrict__ diag, int lds_bodies, const ExactCounts *__restrict__ dc,
                                                      int sched_ints)
{
    solve_island_wg_body<T, WG, REGS, FB, APX>(S, bflags, stride, I, P, diag, lds_bodies, dc, sched_ints, blockIdx.x, gridDim.x);
}
// The tail of a small-scene exact tick in ONE launch: workgroups [0, max_big) are solve_island_wg<64>'s (speculative form: they ask
// the device's record whether their island exists), the workgroups behind them step 64 bodies each of everyone else with the fused
// ground-plane kernel's own code (step_plane_body, dmx_step_fused.hpp; Pf carries the involved bodies' skip mask and the same
// gate).  The two touch disjoint bodies; one after the other they cost 49 + 15 us on a 1 024-body scene, side by side 49.
template <class T>
__global__ __launch_bounds__(64) void solve_islands_and_step(T *__restrict__ S, const uint8_t *__restrict__ bflags,
                                                             const uint8_t *__restrict__ gtype, int64_t stride, int64_t n, IslandSet<T> I,
                                                             StepParams<T> P, StepParams<T> Pf, StepDiag *__restrict__ diag_isl,
                                                             StepDiag *__restrict__ diag_fused, int lds_bodies,
                                                             const ExactCounts *__restrict__ dc, unsigned max_big)
{
    if (blockIdx.x < max_big) solve_island_wg_body<T, 64, false>(S, bflags, stride, I, P, diag_isl, lds_bodies, dc, 0, blockIdx.x, gridDim.x);
    else step_plane_body<T, false, 4>(S, S, gtype, stride, n, Pf, diag_fused, (int64_t)(blockIdx.x - max_big) * 64 + threadIdx.x);
}

// dWorldStep: the islands without rows (free bodies).  Those with rows are solved exactly elsewhere: lcp_island_lds and the
// grid solve, dmx_lcp.hip.
template <class T>
hipError_t launch_islands_without_rows(T *S, const uint8_t *bflags, int64_t stride, const IslandSet<T> &I, const StepParams<T> &P,
                                       StepDiag *diag, hipStream_t st)
{
    if (I.n_islands <= 0) return hipSuccess;
    if (I.n_big < I.n_islands) {
        const unsigned grid = (unsigned)((I.n_islands + 63) / 64);
        hipLaunchKernelGGL((solve_islands<T>), dim3(grid), dim3(64), 0, st, S, bflags, stride, I, P, diag);
    }
    return hipGetLastError();
}

// FB: a tick made with feedback on launches the FB instantiations (row_setup leaves Ad in the rows; I.singles is 0 then)
// APX: a tick with pyramid rows (DMX_CONTACT_APPROX1) launches the APX instantiations, which are made with FB's store on and so
// serve it with feedback on or off (I.singles is 0 then too: the one-body forms know box friction only)
template <class T, bool FB, bool APX = false>
static hipError_t launch_islands_fb(T *S, const uint8_t *bflags, int64_t stride, const IslandSet<T> &I, const StepParams<T> &P,
                                    StepDiag *diag, hipStream_t st)
{
    if (I.n_islands <= 0) return hipSuccess;
    if (I.n_big < I.n_islands) {
        const unsigned grid = (unsigned)((I.n_islands + 63) / 64);
        hipLaunchKernelGGL((solve_islands<T, FB, APX>), dim3(grid), dim3(64), 0, st, S, bflags, stride, I, P, diag);
        if (I.singles) {
            hipLaunchKernelGGL((solve_singles<T>), dim3(grid), dim3(64), 0, st, S, bflags, stride, I, P, diag);
            // islands of 5..8 contacts keep their rows' J and M^-1 J^T in LDS: 64 lanes x 24 rows x 12 fields (f32: 72 KB, two waves
            // per CU; f64: 144 KB of the CU's 160 KB)
            const int lanes = 64;
            const size_t lds = (size_t)lanes * 3 * SINGLE_MAXC_LDS * RS_FIELDS * sizeof(T);
            // (set per launch: the attribute belongs to the function ON THE CURRENT DEVICE, and the call is a table write -- a
            //  process-wide "done once" flag would leave a second device, or a second thread racing the first, without it)
            const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void *>(&solve_singles_lds<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (ea != hipSuccess) return ea;
            hipLaunchKernelGGL((solve_singles_lds<T>), dim3((unsigned)((I.n_islands + lanes - 1) / lanes)), dim3(lanes), lds, st, S, bflags,
                               stride, I, P, diag);
        }
    }
    if (I.n_big > 0) {
        // islands of up to lds_bodies bodies keep their accumulators in LDS (larger ones: HBM/L2)
        const int lds_cap = FC_LDS_BYTES / (int)(6 * sizeof(T));
        const int lds_bodies = std::min<int>(std::max(I.big_max_bodies, 1), lds_cap);
        size_t lds = (size_t)lds_bodies * 6 * sizeof(T);
        // a launch whose largest island has more rows than one wavefront holds but few enough for a workgroup's registers (and not
        // thousands of islands: the form runs one workgroup per compute unit) keeps every island's rows in registers for the sweeps
        // (512 threads, two waves per SIMD: six rows a thread all in the 256 architectural registers -- at 256 threads the same rows
        //  are twelve a thread, half of them in accumulator registers that have to be copied out before every use, and twice the
        //  slots to skip per level; DMX_REGS_WG=256 for that form)
        static const int regs_wg = [] { const char *e = getenv("DMX_REGS_WG"); return e && atoi(e) == 256 ? 256 : 512; }();
        if (I.big_max_rows > WAVE_ISLAND_ROWS && I.big_max_rows <= REGS_ROWS<T> && I.n_big <= 1024) {
            // (f64 rows are 64 registers: three a thread at 512 threads spill; 256 threads, six a thread, do not.  Up to 1 024 rows
            //  256 threads hold them in four slots a thread without the accumulator half, and a level step has four waves to
            //  bring to the barrier, not eight: the pen 96 bodies 264 vs 270 us, 400 bodies 645 vs 583, 512 bodies 961 vs 793)
            // (+ one int per contact behind the accumulators: the contact form's list of contacts in level order)
            static const bool by_contact = [] { const char *e = getenv("DMX_REGS_BY_CONTACT"); return !(e && atoi(e) == 0); }();
            const int scratch = by_contact && sizeof(T) == 4 ? REGS_ROWS<T> / 3 : 0;
            lds += (size_t)scratch * sizeof(int);
            // (a tick with pyramid rows takes the 256-thread form throughout: the 512-thread form's APX instantiation needs 256 VGPRs and
            //  spills, and nothing has measured it; its one word per row of static LDS on top of the accumulators can pass the 64 KB a
            //  launch gets unasked, hence the attribute)
            if constexpr (APX) {
                const hipError_t ea = hipFuncSetAttribute((const void *)&solve_island_wg<T, 256, true, FB, APX>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                if (ea != hipSuccess) return ea;
                hipLaunchKernelGGL((solve_island_wg<T, 256, true, FB, APX>), dim3((unsigned)I.n_big), dim3(256), lds, st, S, bflags, stride, I, P, diag, lds_bodies,
                                   (const ExactCounts *)nullptr, scratch);
            } else if (regs_wg == 512 && sizeof(T) == 4 && I.big_max_rows > 1024)
                hipLaunchKernelGGL((solve_island_wg<T, 512, true, FB, APX>), dim3((unsigned)I.n_big), dim3(512), lds, st, S, bflags, stride, I, P, diag, lds_bodies,
                                   (const ExactCounts *)nullptr, scratch);
            else
                hipLaunchKernelGGL((solve_island_wg<T, 256, true, FB, APX>), dim3((unsigned)I.n_big), dim3(256), lds, st, S, bflags, stride, I, P, diag, lds_bodies,
                                   (const ExactCounts *)nullptr, scratch);
        } else {
            // room for an island's level schedule behind the accumulators (offsets + row lists; big_rows_total bounds any one island's):
            // taken when it is modest -- a few large islands (a pile in the pen) -- not when thousands of small ones share the launch
            const size_t sched = I.big_rows_total > 0 ? (size_t)2 * I.big_rows_total + 2 : 0;
            int sched_ints = 0;
            if (sched > 0 && lds + sched * sizeof(int) <= (size_t)96 * 1024 && I.n_big <= 64) { sched_ints = (int)sched; lds += sched * sizeof(int); }
            if (lds > (size_t)64 * 1024) {
                const void *fn = I.big_max_width <= 64 ? (const void *)&solve_island_wg<T, 64, false, FB, APX> : (const void *)&solve_island_wg<T, 256, false, FB, APX>;
                const hipError_t ea = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                if (ea != hipSuccess) return ea;
            }
            if (I.big_max_width <= 64)      // no level has more than 64 rows: one wavefront per island, barriers cost nothing
                hipLaunchKernelGGL((solve_island_wg<T, 64, false, FB, APX>), dim3((unsigned)I.n_big), dim3(64), lds, st, S, bflags, stride, I, P, diag, lds_bodies, (const ExactCounts *)nullptr, sched_ints);
            else
                hipLaunchKernelGGL((solve_island_wg<T, 256, false, FB, APX>), dim3((unsigned)I.n_big), dim3(256), lds, st, S, bflags, stride, I, P, diag, lds_bodies, (const ExactCounts *)nullptr, sched_ints);
        }
    }
    return hipGetLastError();
}
template <class T>
hipError_t launch_islands(T *S, const uint8_t *bflags, int64_t stride, const IslandSet<T> &I, const StepParams<T> &P,
                          StepDiag *diag, hipStream_t st, bool feedback, bool pyramid)
{
    if (pyramid) return launch_islands_fb<T, true, true>(S, bflags, stride, I, P, diag, st);
    return feedback ? launch_islands_fb<T, true>(S, bflags, stride, I, P, diag, st) : launch_islands_fb<T, false>(S, bflags, stride, I, P, diag, st);
}

// The island solve of a small-scene exact tick, enqueued BEHIND the bookkeeping kernels and before the host has seen their
// counts: one-wavefront workgroups over `max_big` islands (the capacity), every one asking the device's count record whether it
// exists and whether the launch may act (ExactCounts::spec_ok: all islands are solve_island_wg<64>'s kind, nothing overflowed).
// I's counts are not read.
template <class T>
hipError_t launch_islands_speculative(T *S, const uint8_t *bflags, int64_t stride, const IslandSet<T> &I, const StepParams<T> &P,
                                      StepDiag *diag, const ExactCounts *counts_dev, unsigned max_big, hipStream_t st)
{
    if (max_big == 0) return hipSuccess;
    const int lds_bodies = (int)EX_SPEC_ISLAND_BODIES;        // (<= FC_LDS_BYTES' worth: every island of a tick that passes takes the LDS path, as in launch_islands)
    const size_t lds = (size_t)lds_bodies * 6 * sizeof(T);
    hipLaunchKernelGGL((solve_island_wg<T, 64>), dim3(max_big), dim3(64), lds, st, S, bflags, stride, I, P, diag, lds_bodies, counts_dev, 0);
    return hipGetLastError();
}
// ... and the same with the fused ground-plane step for everyone else in the launch (solve_islands_and_step): scenes of boxes and
// spheres on the plane, no static boxes, no hulls, no pending external forces
template <class T>
hipError_t launch_islands_and_step_speculative(T *S, const uint8_t *bflags, const uint8_t *gtype, int64_t stride, int64_t n, const IslandSet<T> &I,
                                               const StepParams<T> &P, const StepParams<T> &Pf, StepDiag *diag_isl, StepDiag *diag_fused,
                                               const ExactCounts *counts_dev, unsigned max_big, hipStream_t st)
{
    const int lds_bodies = (int)EX_SPEC_ISLAND_BODIES;
    const size_t lds = (size_t)lds_bodies * 6 * sizeof(T);
    const unsigned blocks = max_big + (unsigned)((n + 63) / 64);
    hipLaunchKernelGGL((solve_islands_and_step<T>), dim3(blocks), dim3(64), lds, st, S, bflags, gtype, stride, n, I, P, Pf, diag_isl, diag_fused,
                       lds_bodies, counts_dev, max_big);
    return hipGetLastError();
}
template hipError_t launch_islands_and_step_speculative<float>(float *, const uint8_t *, const uint8_t *, int64_t, int64_t, const IslandSet<float> &,
                                                               const StepParams<float> &, const StepParams<float> &, StepDiag *, StepDiag *,
                                                               const ExactCounts *, unsigned, hipStream_t);
template hipError_t launch_islands_and_step_speculative<double>(double *, const uint8_t *, const uint8_t *, int64_t, int64_t, const IslandSet<double> &,
                                                                const StepParams<double> &, const StepParams<double> &, StepDiag *, StepDiag *,
                                                                const ExactCounts *, unsigned, hipStream_t);

template hipError_t launch_islands_speculative<float>(float *, const uint8_t *, int64_t, const IslandSet<float> &, const StepParams<float> &,
                                                      StepDiag *, const ExactCounts *, unsigned, hipStream_t);
template hipError_t launch_islands_speculative<double>(double *, const uint8_t *, int64_t, const IslandSet<double> &, const StepParams<double> &,
                                                       StepDiag *, const ExactCounts *, unsigned, hipStream_t);

template hipError_t launch_islands_without_rows<float>(float *, const uint8_t *, int64_t, const IslandSet<float> &,
                                                       const StepParams<float> &, StepDiag *, hipStream_t);
template hipError_t launch_islands_without_rows<double>(double *, const uint8_t *, int64_t, const IslandSet<double> &,
                                                        const StepParams<double> &, StepDiag *, hipStream_t);
template hipError_t launch_islands<float>(float *, const uint8_t *, int64_t, const IslandSet<float> &,
                                          const StepParams<float> &, StepDiag *, hipStream_t, bool, bool);
template hipError_t launch_islands<double>(double *, const uint8_t *, int64_t, const IslandSet<double> &,
                                           const StepParams<double> &, StepDiag *, hipStream_t, bool, bool);

// HIP loads a translation unit's code object at the first launch of one of its kernels -- a couple of milliseconds each, which an
// interactive caller would meet as a hitch at the first tick that needs the exact pipeline.  dmxBatchCreate asks for one
// kernel's attributes per unit instead (dmx_preload_code, dmx_batch.cpp): the load happens there.
hipError_t dmx_touch_islands(int real_bytes)
{
    // (the unit's code object, and -- what costs more -- each kernel's own first-use set-up: every kernel an exact tick or a fused
    //  tick may launch, in the batch's precision)
    hipFuncAttributes a;
    hipError_t e = hipSuccess;
    auto touch = [&](const void *k) { const hipError_t r = hipFuncGetAttributes(&a, k); if (r != hipSuccess) e = r; };
    if (real_bytes == 4) {
        touch((const void *)&solve_islands<float>);
        touch((const void *)&solve_singles<float>);
        touch((const void *)&solve_singles_lds<float>);
        touch((const void *)&solve_island_wg<float, 64, false>);
        touch((const void *)&solve_island_wg<float, 256, false>);
        touch((const void *)&solve_island_wg<float, 256, true>);
        touch((const void *)&solve_island_wg<float, 512, true>);
        touch((const void *)&solve_islands_and_step<float>);
    } else {
        touch((const void *)&solve_islands<double>);
        touch((const void *)&solve_singles<double>);
        touch((const void *)&solve_singles_lds<double>);
        touch((const void *)&solve_island_wg<double, 64, false>);
        touch((const void *)&solve_island_wg<double, 256, false>);
        touch((const void *)&solve_island_wg<double, 256, true>);
        touch((const void *)&solve_island_wg<double, 512, true>);
        touch((const void *)&solve_islands_and_step<double>);
    }
    return e;
}

}  // namespace dmx
