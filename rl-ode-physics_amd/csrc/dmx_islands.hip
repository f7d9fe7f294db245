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
template <class T>
__global__ __launch_bounds__(64) void solve_islands(T *__restrict__ S, const uint8_t *__restrict__ bflags,
                                                    int64_t stride, IslandSet<T> I, StepParams<T> P,
                                                    StepDiag *__restrict__ diag)
{
    solve_islands_body<T>(S, bflags, stride, I, P, diag, (int)(blockIdx.x * blockDim.x + threadIdx.x));
}
template <class T, int WG, bool REGS = false>
__global__ __launch_bounds__(WG) void solve_island_wg(T *__restrict__ S, const uint8_t *__restrict__ bflags,
                                                      int64_t stride, IslandSet<T> I, StepParams<T> P,
                                                      StepDiag *__restrict__ diag, int lds_bodies, const ExactCounts *__restrict__ dc,
                                                      int sched_ints)
{
    solve_island_wg_body<T, WG, REGS>(S, bflags, stride, I, P, diag, lds_bodies, dc, sched_ints, blockIdx.x, gridDim.x);
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

// ================================================================================ dWorldStep: the island's LCP solved exactly
// One workgroup per island with rows.  Same rows as the SOR kernels (stage_body / contact_rows / body_tmp / row_setup),
// then  A = J M^-1 J^T + diag(cfm / h)  and block principal pivoting on  A lambda = b + w, lo <= lambda <= hi  (free /
// at-lo / at-hi sets, Cholesky of the free block, flip the violators; Murty's single flip once the violation count has
// stalled three times); every loop has a fixed operation order, whatever the thread mapping.  A lives in HBM/L2 (m^2 reals
// per island, scratch sized by the host); the free block's factor is staged in LDS when it fits.
enum : int { LCP_FREE = 0, LCP_LO = 1, LCP_HI = 2 };

template <class T> __device__ __forceinline__ T dot6acc(const T *a, const T *b, T acc)
{
#pragma unroll
    for (int k = 0; k < 6; k++) acc = fma_(a[k], b[k], acc);
    return acc;
}

template <class T, int WG>
__global__ __launch_bounds__(WG) void lcp_island_wg(T *__restrict__ S, const uint8_t *__restrict__ bflags, int64_t stride,
                                                    IslandSet<T> I, StepParams<T> P, StepDiag *__restrict__ diag,
                                                    T *__restrict__ scratch, const long long *__restrict__ scratch_off,
                                                    int *__restrict__ iscratch, int lds_rows)
{
    const int isl = I.big_list[blockIdx.x];
    const int tid = threadIdx.x;
    const T h = P.h, hinv = T(1) / h;
    const int b0 = I.body_off[isl], nb = I.body_off[isl + 1] - b0;
    const int c0 = I.con_off[isl], nc = I.con_off[isl + 1] - c0;
    const int r0 = I.row_off[isl];
    T *bs = I.bscr + (size_t)b0 * BW_COUNT;
    T *rows = I.rows + (size_t)r0 * RW_COUNT;
    int *jb = I.rowjb + 2 * (size_t)r0;
    // rows of this island: contacts are laid out by crow (first row of each contact), rpc rows each
    const int m = nc > 0 ? I.crow[c0 + nc - 1] + contact_rpc(I, P, c0 + nc - 1) : 0;

    for (int k = tid; k < nb; k += WG) stage_body(S, bflags, stride, I, P, bs + (size_t)k * BW_COUNT, I.bodies[b0 + k], k);
    __syncthreads();
    for (int c = tid; c < nc; c += WG) contact_rows(S, stride, I, P, rows, jb, c0 + c, I.crow[c0 + c], hinv);
    for (int k = tid; k < nb; k += WG) body_tmp(S, stride, bs + (size_t)k * BW_COUNT, I.bodies[b0 + k], hinv);
    __syncthreads();
    for (int i = tid; i < m; i += WG) row_setup<T, false>(rows, jb, bs, i, hinv, P.sor_w);
    __syncthreads();

    T *A = scratch + scratch_off[blockIdx.x];
    T *Mg = A + (size_t)m * m, *rg = Mg + (size_t)m * m, *lam = rg + m, *wv = lam + m;
    int *state = iscratch + 3 * (size_t)r0, *idx = state + m, *viol = idx + m;
    extern __shared__ __align__(16) unsigned char lcp_raw[];
    __shared__ int s_nf, s_done;
    __shared__ T s_tol;

    // A = J iMJ^T over shared bodies + diag(cfm / h)
    for (long long e = tid; e < (long long)m * m; e += WG) {
        const int i = (int)(e / m), j = (int)(e - (long long)i * m);
        const T *ji = rows + (size_t)i * RW_COUNT + RW_J, *pj = rows + (size_t)j * RW_COUNT + RW_IMJ;
        const int i1 = jb[2 * i], i2 = jb[2 * i + 1], j1 = jb[2 * j], j2 = jb[2 * j + 1];
        T a = T(0);
        if (i1 == j1) a = dot6acc(ji, pj, a);
        if (j2 >= 0 && i1 == j2) a = dot6acc(ji, pj + 6, a);
        if (i2 >= 0 && i2 == j1) a = dot6acc(ji + 6, pj, a);
        if (i2 >= 0 && j2 >= 0 && i2 == j2) a = dot6acc(ji + 6, pj + 6, a);
        if (i == j) a += rows[(size_t)i * RW_COUNT + RW_AD];
        A[e] = a;
    }
    if (tid == 0) {
        T bmax = T(0);
        for (int i = 0; i < m; i++) { const T v = tabs(rows[(size_t)i * RW_COUNT + RW_RHS]); if (v > bmax) bmax = v; }
        s_tol = (sizeof(T) == 4 ? T(1e-5) : T(1e-11)) * (T(1) + bmax);
    }
    for (int i = tid; i < m; i += WG) { state[i] = LCP_FREE; lam[i] = T(0); }
    __syncthreads();
    const T tol = s_tol;
    int best = m + 1, patience = 3;                     // (only thread 0's copies matter)
    bool single = false;
    const int max_rounds = 20 * m + 100;
    for (int round = 0;; round++) {
        if (tid == 0) {
            int nf = 0;
            for (int i = 0; i < m; i++) {
                if (state[i] == LCP_FREE) idx[nf++] = i;
                else lam[i] = state[i] == LCP_LO ? rows[(size_t)i * RW_COUNT + RW_LO] : rows[(size_t)i * RW_COUNT + RW_HI];
            }
            s_nf = nf;
        }
        __syncthreads();
        const int nf = s_nf;
        const bool in_lds = nf <= lds_rows;             // the free block's factor and right-hand side fit in LDS
        T *M = in_lds ? reinterpret_cast<T *>(lcp_raw) : Mg;
        T *r = in_lds ? M + (size_t)nf * nf : rg;
        for (int a = tid; a < nf; a += WG) {
            const int i = idx[a];
            T s = rows[(size_t)i * RW_COUNT + RW_RHS];
            for (int j = 0; j < m; j++) if (state[j] != LCP_FREE && lam[j] != T(0)) s -= A[(size_t)i * m + j] * lam[j];
            r[a] = s;
        }
        for (long long e = tid; e < (long long)nf * nf; e += WG) {
            const int a = (int)(e / nf), c = (int)(e - (long long)a * nf);
            if (c <= a) M[e] = A[(size_t)idx[a] * m + idx[c]];
        }
        __syncthreads();
        // Cholesky, right-looking, lower triangle in place
        for (int k = 0; k < nf; k++) {
            if (tid == 0) { T d = M[(size_t)k * nf + k]; d = tsqrt<T>(d > T(0) ? d : tol); M[(size_t)k * nf + k] = d; }
            __syncthreads();
            const T d = M[(size_t)k * nf + k];
            for (int i = k + 1 + tid; i < nf; i += WG) M[(size_t)i * nf + k] /= d;
            __syncthreads();
            const int cnt = nf - k - 1;
            const long long total = (long long)cnt * (cnt + 1) / 2;
            for (long long e = tid; e < total; e += WG) {
                int ii = (int)((tsqrt<double>(8.0 * (double)e + 1.0) - 1.0) * 0.5);
                while ((long long)ii * (ii + 1) / 2 > e) ii--;
                while ((long long)(ii + 1) * (ii + 2) / 2 <= e) ii++;
                const int jj = (int)(e - (long long)ii * (ii + 1) / 2);
                const int i = k + 1 + ii, j = k + 1 + jj;
                M[(size_t)i * nf + j] -= M[(size_t)i * nf + k] * M[(size_t)j * nf + k];
            }
            __syncthreads();
        }
        // L y = r (column oriented), L^T x = y
        for (int k = 0; k < nf; k++) {
            if (tid == 0) r[k] /= M[(size_t)k * nf + k];
            __syncthreads();
            const T rk = r[k];
            for (int i = k + 1 + tid; i < nf; i += WG) r[i] -= M[(size_t)i * nf + k] * rk;
            __syncthreads();
        }
        for (int k = nf - 1; k >= 0; k--) {
            if (tid == 0) r[k] /= M[(size_t)k * nf + k];
            __syncthreads();
            const T rk = r[k];
            for (int i = tid; i < k; i += WG) r[i] -= M[(size_t)k * nf + i] * rk;
            __syncthreads();
        }
        for (int a = tid; a < nf; a += WG) lam[idx[a]] = r[a];
        __syncthreads();
        for (int i = tid; i < m; i += WG) {
            T s = -rows[(size_t)i * RW_COUNT + RW_RHS];
            for (int j = 0; j < m; j++) s += A[(size_t)i * m + j] * lam[j];
            wv[i] = s;
        }
        __syncthreads();
        if (tid == 0) {
            int nv = 0, top = -1;
            for (int i = 0; i < m; i++) {
                const T lo = rows[(size_t)i * RW_COUNT + RW_LO], hi = rows[(size_t)i * RW_COUNT + RW_HI];
                int v = 0;
                if (state[i] == LCP_FREE) v = (lam[i] < lo - tol) ? 1 : (lam[i] > hi + tol) ? 2 : 0;
                else if (state[i] == LCP_LO) v = wv[i] < -tol ? 3 : 0;
                else v = wv[i] > tol ? 3 : 0;
                viol[i] = v;
                if (v) { nv++; top = i; }
            }
            int done = (nv == 0 || round >= max_rounds) ? 1 : 0;
            if (!done) {
                if (nv < best) { best = nv; if (!single) patience = 3; }      // single flips, once begun, to the end
                else if (patience > 0) patience--;
                else single = true;
                const bool all = !single;
                for (int i = 0; i < m; i++) {
                    if (!viol[i] || (!all && i != top)) continue;
                    state[i] = viol[i] == 1 ? LCP_LO : viol[i] == 2 ? LCP_HI : LCP_FREE;
                }
            }
            s_done = done;
        }
        __syncthreads();
        if (s_done) break;
    }
    // clamp what the tolerance let through; cforce = M^-1 J^T lambda, rows in order per body
    for (int i = tid; i < m; i += WG) {
        T l = lam[i];
        if (state[i] == LCP_FREE) {
            const T lo = rows[(size_t)i * RW_COUNT + RW_LO], hi = rows[(size_t)i * RW_COUNT + RW_HI];
            if (l < lo) l = lo;
            if (l > hi) l = hi;
        }
        lam[i] = l;
        rows[(size_t)i * RW_COUNT + RW_LAM] = l;
    }
    __syncthreads();
    double resid = 0.0;
    for (int k = tid; k < nb; k += WG) {
        T f[6] = { T(0), T(0), T(0), T(0), T(0), T(0) };
        for (int i = 0; i < m; i++) {
            const T *ip = rows + (size_t)i * RW_COUNT + RW_IMJ;
            if (jb[2 * i] == k) { for (int q = 0; q < 6; q++) f[q] = fma_(lam[i], ip[q], f[q]); }
            if (jb[2 * i + 1] == k) { for (int q = 0; q < 6; q++) f[q] = fma_(lam[i], ip[6 + q], f[q]); }
        }
        for (int q = 0; q < 6; q++) bs[(size_t)k * BW_COUNT + BW_FC + q] = f[q];
    }
    for (int i = tid; i < m; i += WG) {
        const T w_i = wv[i];
        resid += (double)(state[i] == LCP_FREE ? tabs(w_i) : (state[i] == LCP_LO ? (w_i < T(0) ? -w_i : T(0)) : (w_i > T(0) ? w_i : T(0))));
    }
    for (int k = tid; k < nb; k += WG) finish_body(S, bflags, stride, bs + (size_t)k * BW_COUNT, I.bodies[b0 + k], m > 0, h);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) resid += __shfl_xor(resid, o, 64);
    if ((tid & 63) == 0) atomicAdd(&diag->residual, resid);
    if (tid == 0) atomicAdd(&diag->contacts, (unsigned long long)nc);
}

template <class T>
hipError_t launch_islands_exact(T *S, const uint8_t *bflags, int64_t stride, const IslandSet<T> &I, const StepParams<T> &P,
                                StepDiag *diag, T *scratch, const long long *scratch_off, int *iscratch, int max_rows, hipStream_t st)
{
    // (max_rows < 0: the caller solves the islands with rows itself -- lcp_island_lds, dmx_lcp.hip -- and wants the row-less ones only)
    if (I.n_islands <= 0) return hipSuccess;
    if (I.n_big < I.n_islands) {       // islands without rows: free bodies
        const unsigned grid = (unsigned)((I.n_islands + 63) / 64);
        hipLaunchKernelGGL((solve_islands<T>), dim3(grid), dim3(64), 0, st, S, bflags, stride, I, P, diag);
    }
    if (I.n_big > 0 && max_rows >= 0) {
        // LDS for the free block's factor + right-hand side, up to 60 KB
        int lds_rows = 0;
        while ((size_t)(lds_rows + 1) * (lds_rows + 2) * sizeof(T) <= (size_t)60 * 1024 && lds_rows < max_rows) lds_rows++;
        const size_t lds = (size_t)lds_rows * (lds_rows + 1) * sizeof(T);
        hipLaunchKernelGGL((lcp_island_wg<T, 256>), dim3((unsigned)I.n_big), dim3(256), lds, st, S, bflags, stride, I, P, diag,
                           scratch, scratch_off, iscratch, lds_rows);
    }
    return hipGetLastError();
}

template <class T>
hipError_t launch_islands(T *S, const uint8_t *bflags, int64_t stride, const IslandSet<T> &I, const StepParams<T> &P,
                          StepDiag *diag, hipStream_t st)
{
    if (I.n_islands <= 0) return hipSuccess;
    if (I.n_big < I.n_islands) {
        const unsigned grid = (unsigned)((I.n_islands + 63) / 64);
        hipLaunchKernelGGL((solve_islands<T>), dim3(grid), dim3(64), 0, st, S, bflags, stride, I, P, diag);
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
            if (regs_wg == 512 && sizeof(T) == 4 && I.big_max_rows > 1024)
                hipLaunchKernelGGL((solve_island_wg<T, 512, true>), dim3((unsigned)I.n_big), dim3(512), lds, st, S, bflags, stride, I, P, diag, lds_bodies,
                                   (const ExactCounts *)nullptr, scratch);
            else
                hipLaunchKernelGGL((solve_island_wg<T, 256, true>), dim3((unsigned)I.n_big), dim3(256), lds, st, S, bflags, stride, I, P, diag, lds_bodies,
                                   (const ExactCounts *)nullptr, scratch);
        } else {
            // room for an island's level schedule behind the accumulators (offsets + row lists; big_rows_total bounds any one island's):
            // taken when it is modest -- a few large islands (a pile in the pen) -- not when thousands of small ones share the launch
            const size_t sched = I.big_rows_total > 0 ? (size_t)2 * I.big_rows_total + 2 : 0;
            int sched_ints = 0;
            if (sched > 0 && lds + sched * sizeof(int) <= (size_t)96 * 1024 && I.n_big <= 64) { sched_ints = (int)sched; lds += sched * sizeof(int); }
            if (lds > (size_t)64 * 1024) {
                const void *fn = I.big_max_width <= 64 ? (const void *)&solve_island_wg<T, 64, false> : (const void *)&solve_island_wg<T, 256, false>;
                const hipError_t ea = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                if (ea != hipSuccess) return ea;
            }
            if (I.big_max_width <= 64)      // no level has more than 64 rows: one wavefront per island, barriers cost nothing
                hipLaunchKernelGGL((solve_island_wg<T, 64>), dim3((unsigned)I.n_big), dim3(64), lds, st, S, bflags, stride, I, P, diag, lds_bodies, (const ExactCounts *)nullptr, sched_ints);
            else
                hipLaunchKernelGGL((solve_island_wg<T, 256>), dim3((unsigned)I.n_big), dim3(256), lds, st, S, bflags, stride, I, P, diag, lds_bodies, (const ExactCounts *)nullptr, sched_ints);
        }
    }
    return hipGetLastError();
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

template hipError_t launch_islands_exact<float>(float *, const uint8_t *, int64_t, const IslandSet<float> &, const StepParams<float> &,
                                                StepDiag *, float *, const long long *, int *, int, hipStream_t);
template hipError_t launch_islands_exact<double>(double *, const uint8_t *, int64_t, const IslandSet<double> &, const StepParams<double> &,
                                                 StepDiag *, double *, const long long *, int *, int, hipStream_t);
template hipError_t launch_islands<float>(float *, const uint8_t *, int64_t, const IslandSet<float> &,
                                          const StepParams<float> &, StepDiag *, hipStream_t);
template hipError_t launch_islands<double>(double *, const uint8_t *, int64_t, const IslandSet<double> &,
                                           const StepParams<double> &, StepDiag *, hipStream_t);

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
