// dmx_lcp_lds.hpp -- dWorldStep's one-workgroup exact island solve, the whole LCP in LDS, as a device function
// (lcp_island_lds_body) with its helpers.  The kernel lcp_island_lds of dmx_lcp.hip is a thin wrapper; the single-launch tick
// of small worlds (dmx_small.hip) calls the same function.
#pragma once

#include <hip/hip_runtime.h>
#include "dmx_internal.hpp"
#include "dmx_math.hpp"
#include "dmx_island_rows.hpp"

namespace dmx {
namespace {

enum : int { ST_FREE = 0, ST_LO = 1, ST_HI = 2 };

// =========================================================================================================== small and medium islands
// One workgroup per island, the whole solve in LDS: the same method as the grid solve above (never-clamping rows first, eliminated
// once; block principal pivoting on the Schur complement in the bounded rows; lambda_U by back-substitution), as an LDL^T on a
// packed lower triangle -- no square roots and ONE barrier per pivot: at step k every thread reads the pivot M(k,k) and the column
// below it, which the previous step's barrier made final, and updates its share of the trailing triangle
//   M(i,j) -= M(i,k) M(j,k) / M(k,k),   i > k, k < j <= i;
// column k stays as it is (c_ik = l_ik d_k), the right-hand side rides along as the last row (it ends as y = L^-1 b).
// Islands of up to a few hundred rows in the reference's pen while the pile is still loose (/root/reference/src/main.c:213).
__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }      // j <= i

// steps [k0, k1) of the LDL^T of the packed matrix M whose rows 0 .. last are stored (row `last` = the right-hand side; the
// unknowns are rows / columns 0 .. last - 1); dinv[k] = 1 / pivot.  Ends with a barrier.
// FOUR pivots a pass (round 4; one a pass before: a 93-row solve was 93 passes of a few hundred cycles' work between two barriers,
// 0.2 us each whatever the work, and the volatile rows' solve refactors ten times a call).  A pass: (A) every thread eliminates the
// 4 x 4 pivot block for itself (ten values, read before anybody writes them), and the thread that owns a row below the block brings
// the row's four panel entries up to date -- entry q by the pivots before q, exactly the products the one-pivot passes made, in
// their order -- leaves them in the matrix and in a small buffer; barrier; (B) the trailing triangle takes the four updates of
// every element in one read-modify-write; barrier.  Same operands, same order per element: same bits.
template <class T> constexpr int LDLT_MAXN = sizeof(T) == 8 ? 192 : 288;       // rows (the right-hand side's included) an LDS solve holds at most
template <class T, int WG>
__device__ __forceinline__ void ldlt_steps(T *M, int last, int k0, int k1, T *dinv, T tol, int tid)
{
    constexpr int NBK = 4;
    __shared__ T pn[LDLT_MAXN<T>][NBK];
    const int ty = tid >> 4, tx = tid & 15;
    for (int k = k0; k < k1; k += NBK) {
        const int nb = k1 - k < NBK ? k1 - k : NBK;
        // ---- (A) the pivot block, by everybody
        T A[NBK][NBK], inv[NBK];
#pragma unroll
        for (int p = 0; p < NBK; p++)
#pragma unroll
            for (int q = 0; q <= p; q++) A[p][q] = p < nb ? M[tri(k + p, k + q)] : T(0);
#pragma unroll
        for (int q = 0; q < NBK; q++) {
            T d = A[q][q];
            d = d > T(0) ? d : tol;               // (the oracle's guard: a pivot that rounding pushed below zero)
            inv[q] = T(1) / d;
#pragma unroll
            for (int p = q + 1; p < NBK; p++) {
                const T c = A[p][q] * inv[q];
#pragma unroll
                for (int j = q + 1; j <= p; j++) A[p][j] = fma_(-c, A[j][q], A[p][j]);
            }
        }
        if (tid < nb) dinv[k + tid] = tid == 0 ? inv[0] : tid == 1 ? inv[1] : tid == 2 ? inv[2] : inv[3];
        // the rows below the block: their panel entries
        for (int i = k + nb + tid; i <= last; i += WG) {
            T *Mi = M + tri(i, k);
            T r[NBK];
#pragma unroll
            for (int q = 0; q < NBK; q++) r[q] = q < nb ? Mi[q] : T(0);
#pragma unroll
            for (int q = 0; q < NBK; q++) {
                const T c = r[q] * inv[q];
#pragma unroll
                for (int j = q + 1; j < NBK; j++) r[j] = fma_(-c, A[j][q], r[j]);
            }
#pragma unroll
            for (int q = 0; q < NBK; q++) { pn[i][q] = r[q]; if (q >= 1 && q < nb) Mi[q] = r[q]; }
        }
        __syncthreads();
        // ---- (B) the block's own rows keep their final values; the trailing triangle
        if (tid >= 1 && tid < nb) {
            T *Mp = M + tri(k + tid, k);
#pragma unroll
            for (int p = 1; p < NBK; p++)
                if (tid == p) {
#pragma unroll
                    for (int q = 1; q <= p; q++) Mp[q] = A[p][q];
                }
        }
        for (int i = k + nb + ty; i <= last; i += WG / 16) {
            T c[NBK];
#pragma unroll
            for (int q = 0; q < NBK; q++) c[q] = pn[i][q] * inv[q];
            T *Mi = M + tri(i, 0);
            const int jmax = i < last ? i : last - 1;
            for (int j = k + nb + tx; j <= jmax; j += 16) {
                T v = Mi[j];
#pragma unroll
                for (int q = 0; q < NBK; q++)
                    if (q < nb) v = fma_(-c[q], pn[j][q], v);
                Mi[j] = v;
            }
        }
        __syncthreads();
    }
}
// L^T x = z in place over unknowns [0, n) of a packed LDL^T (L(i,k) = M(i,k) dinv[k]); z in LDS.  Ends with a barrier.
// Every z[k] takes its updates in descending i, one product each: 64 unknowns at a time, their own triangle by one wavefront
// (a lane an unknown, the solved value handed round by a shuffle: no barrier per unknown), then everybody below takes the 64.
template <class T, int WG>
__device__ __forceinline__ void ldlt_backsub(const T *M, int n, const T *dinv, T *z, int tid)
{
    const int lane = tid & 63;
    for (int e = n; e > 0; e -= 64) {
        const int s = e > 64 ? e - 64 : 0;
        if (tid < 64) {
            const int k = s + lane;
            T zk = k < e ? z[k] : T(0);
            const T dk = k < e ? dinv[k] : T(0);
            for (int i = e - 1; i > s; i--) {
                const T xi = __shfl(zk, i - s, 64);
                if (k < i) zk = fma_(-M[tri(i, k)] * dk, xi, zk);
            }
            if (k < e) z[k] = zk;
        }
        __syncthreads();
        for (int k = tid; k < s; k += WG) {
            T zk = z[k];
            const T dk = dinv[k];
            for (int i = e - 1; i >= s; i--) zk = fma_(-M[tri(i, k)] * dk, z[i], zk);
            z[k] = zk;
        }
        __syncthreads();
    }
}

// Block principal pivoting on the bounded rows' problem held in LDS: S = rows / columns nu .. nu + nbd - 1 of the packed matrix M,
// b' = its row m from column nu.  state: in = where the active set starts, out = where it ended; lam / wv: the solution and
// w = S lam - b'.  W: room for a packed (nbd + 1)-row matrix; rd: 2 nbd reals.  The oracle's rule: every violating row flips;
// when the count of violations has failed to shrink three times, only the highest violating row does (Murty).  Returns the
// number of rounds.  Ends after a barrier.
template <class T, int WG>
__device__ __forceinline__ int lds_pivot_rounds(const T *M, int m, int nu, int nbd, T *W, T *lam, T *wv, const T *lo, const T *hi, int *state,
                                                int *fidx, int *viol, T *rd, T tol, int murty_only, int max_rounds, int tid)
{
    __shared__ int s_cnt[2][WG / 64 + 1];
    __shared__ int s_nv, s_top;
    const int lane = tid & 63, wave = tid >> 6;
    int round = 0;
    int best = m + 1, patience = murty_only ? 0 : 3;
    bool single = false;
    if (nbd <= 0) return 0;
    for (;; round++) {
        // the free rows in order
        int nf = 0;
        {
            int fbase = 0;
            for (int base = 0; base < nbd; base += WG) {
                const int q = base + tid;
                const bool f = q < nbd && state[q] == ST_FREE;
                const unsigned long long bf = __ballot(f);
                if (lane == 0) s_cnt[0][wave] = __popcll(bf);
                __syncthreads();
                int off = fbase;
                for (int e = 0; e < wave; e++) off += s_cnt[0][e];
                if (f) fidx[off + __popcll(bf & ((1ull << lane) - 1ull))] = q;
                else if (q < nbd) lam[q] = state[q] == ST_LO ? lo[q] : hi[q];
                for (int e = 0; e < WG / 64; e++) fbase += s_cnt[0][e];
                __syncthreads();
            }
            nf = fbase;
        }
        // W = S[F, F] with the right-hand side b'_F - S_FC lambda_C as its last row
        for (int a = tid; a < nf; a += WG) {
            T *Wa = W + tri(a, 0);
            const int qa = fidx[a];
            for (int c = 0; c <= a; c++) Wa[c] = M[tri(nu + qa, nu + fidx[c])];
        }
        for (int c = tid; c <= nf; c += WG) {
            T r = T(0);
            if (c < nf) {
                const int qc = fidx[c];
                r = M[tri(m, nu + qc)];
                for (int e = 0; e < nbd; e++)
                    if (state[e] != ST_FREE && lam[e] != T(0)) r = fma_(-(e >= qc ? M[tri(nu + e, nu + qc)] : M[tri(nu + qc, nu + e)]), lam[e], r);
            }
            W[tri(nf, c)] = r;
        }
        __syncthreads();
        ldlt_steps<T, WG>(W, nf, 0, nf, rd, tol, tid);
        T *x = rd + nbd;          // (z has room for max(nu, 2 nbd))
        for (int a = tid; a < nf; a += WG) x[a] = W[tri(nf, a)] * rd[a];
        __syncthreads();
        ldlt_backsub<T, WG>(W, nf, rd, x, tid);
        for (int a = tid; a < nf; a += WG) lam[fidx[a]] = x[a];
        __syncthreads();
        // w_B = S lambda_B - b', verdicts
        if (tid == 0) { s_nv = 0; s_top = -1; }
        __syncthreads();
        for (int q = tid; q < nbd; q += WG) {
            T sacc = -M[tri(m, nu + q)];
            for (int e = 0; e < nbd; e++) sacc = fma_(e <= q ? M[tri(nu + q, nu + e)] : M[tri(nu + e, nu + q)], lam[e], sacc);
            wv[q] = sacc;
            const int st = state[q];
            int vi = 0;
            if (st == ST_FREE) vi = (lam[q] < lo[q] - tol) ? 1 : (lam[q] > hi[q] + tol) ? 2 : 0;
            else if (st == ST_LO) vi = sacc < -tol ? 3 : 0;
            else vi = sacc > tol ? 3 : 0;
            viol[q] = vi;
            if (vi) { atomicAdd(&s_nv, 1); atomicMax(&s_top, q); }
        }
        __syncthreads();
        const int nviol = s_nv, top = s_top;
        if (nviol == 0 || round >= max_rounds) break;
        // once block pivoting has stalled, Murty's single flips to the end: going back to block flips when a single flip has
        // lowered the count lets the two undo each other, and the solve cycles to max_rounds (masses 1e-3 .. 1e3 in one chain,
        // tests/test_gpu_solver_dense.py)
        if (nviol < best) { best = nviol; if (!murty_only && !single) patience = 3; }
        else if (patience > 0) patience--;
        else single = true;
        const bool all = !(murty_only || single);
        for (int q = tid; q < nbd; q += WG) {
            const int vi = viol[q];
            if (!vi || (!all && q != top)) continue;
            state[q] = vi == 1 ? ST_LO : vi == 2 ? ST_HI : ST_FREE;
        }
        __syncthreads();
    }
    return round + 1;
}

// LDS of lcp_island_lds: M (m + 1 packed rows), W (nbd + 1), lam / w / lo / hi [nbd], dinv [nu], z [max(nu, 2 nbd)]; then the ints
__host__ __device__ inline size_t lcp_lds_reals(int m, int nbd)
{
    const int nu = m - nbd;
    return (size_t)(m + 1) * (m + 2) / 2 + (size_t)(nbd + 1) * (nbd + 2) / 2 + (size_t)4 * nbd + (size_t)nu + (size_t)(nu > 2 * nbd ? nu : 2 * nbd) + 8;
}
template <class T> __host__ __device__ inline size_t lcp_lds_bytes(int m, int nbd)
{
    return ((lcp_lds_reals(m, nbd) * sizeof(T) + 15) / 16) * 16 + ((size_t)3 * m + (size_t)3 * nbd + 16) * sizeof(int);
}

// APX (a tick with pyramid rows, DMX_CONTACT_APPROX1: an instantiation of its own): contact_rows builds the pyramid rows with lo = hi = 0,
// so the pivoting below is the definition's pass A; an island that has such a row then takes their bounds -/+ mu lambda^A_n from the
// normal rows' multipliers and pivots again from the all-free set (pass B: same matrix, same factor of the never-clamping block --
// pyramid rows are bounded rows).  An island without one is solved once.
template <class T, int WG, bool APX = false>
__device__ __forceinline__ void lcp_island_lds_body(T *__restrict__ S, const uint8_t *__restrict__ bflags, int64_t stride, const IslandSet<T> &I,
                                                    const StepParams<T> &P, StepDiag *__restrict__ diag, int murty_only, T tol_rel, unsigned bidx)
{
    const int isl = I.big_list[bidx];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const T h = P.h, hinv = T(1) / h;
    const int b0 = I.body_off[isl], nb = I.body_off[isl + 1] - b0;
    const int c0 = I.con_off[isl], nc = I.con_off[isl + 1] - c0;
    const int r0 = I.row_off[isl];
    T *bs = I.bscr + (size_t)b0 * BW_COUNT;
    T *rows = I.rows + (size_t)r0 * RW_COUNT;
    int *jb = I.rowjb + 2 * (size_t)r0;
    const int m = nc > 0 ? I.crow[c0 + nc - 1] + contact_rpc(I, P, c0 + nc - 1) : 0;

    for (int k = tid; k < nb; k += WG) stage_body(S, bflags, stride, I, P, bs + (size_t)k * BW_COUNT, I.bodies[b0 + k], k);
    __syncthreads();
    for (int c = tid; c < nc; c += WG) contact_rows<T, 0, APX>(S, stride, I, P, rows, jb, c0 + c, I.crow[c0 + c], hinv);
    for (int k = tid; k < nb; k += WG) body_tmp(S, stride, bs + (size_t)k * BW_COUNT, I.bodies[b0 + k], hinv);
    __syncthreads();
    __shared__ int s_cnt[2][WG / 64 + 1];
    __shared__ T s_red[WG / 64];
    // rows: setup, the largest |rhs| (the tolerance's scale), and who can never clamp
    T bmax = T(0);
    for (int i = tid; i < m; i += WG) {
        row_setup<T, false>(rows, jb, bs, i, hinv, P.sor_w);
        const T v = tabs(rows[(size_t)i * RW_COUNT + RW_RHS]);
        if (v > bmax) bmax = v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const T v = __shfl_xor(bmax, o, 64); if (v > bmax) bmax = v; }
    if (lane == 0) s_red[wave] = bmax;
    __syncthreads();
    bmax = s_red[0];
    for (int q = 1; q < WG / 64; q++) if (s_red[q] > bmax) bmax = s_red[q];
    const T tol = tol_rel * (T(1) + bmax);

    extern __shared__ __align__(16) unsigned char lcp_lds_raw[];
    // ---- the permutation: unbounded rows first (m <= a few hundred: passes of WG rows, ballot ranks)
    int nu = 0;
    {
        // count first, then place: two passes over the rows, each with per-wave ballots
        int mine_u = 0;
        for (int base = 0; base < m; base += WG) {
            const int i = base + tid;
            const bool u = i < m && rows[(size_t)i * RW_COUNT + RW_LO] == -Limits<T>::inf() && rows[(size_t)i * RW_COUNT + RW_HI] == Limits<T>::inf();
            const unsigned long long bal = __ballot(u);
            if (lane == 0) mine_u += __popcll(bal);
        }
        if (lane == 0) s_cnt[0][wave] = mine_u;
        __syncthreads();
        for (int q = 0; q < WG / 64; q++) nu += s_cnt[0][q];
        __syncthreads();
    }
    const int nbd = m - nu;
    T *M = reinterpret_cast<T *>(lcp_lds_raw);
    T *W = M + (size_t)(m + 1) * (m + 2) / 2;
    T *lam = W + (size_t)(nbd + 1) * (nbd + 2) / 2, *wv = lam + nbd, *lo = wv + nbd, *hi = lo + nbd;
    T *dinv = hi + nbd, *z = dinv + nu;
    int *perm = reinterpret_cast<int *>(lcp_lds_raw + ((lcp_lds_reals(m, nbd) * sizeof(T) + 15) / 16) * 16);
    int *pb1 = perm + m, *pb2 = pb1 + m, *state = pb2 + m, *fidx = state + nbd, *viol = fidx + nbd;
    {
        int ubase = 0, bbase = 0;
        for (int base = 0; base < m; base += WG) {
            const int i = base + tid;
            const bool in = i < m;
            const bool u = in && rows[(size_t)i * RW_COUNT + RW_LO] == -Limits<T>::inf() && rows[(size_t)i * RW_COUNT + RW_HI] == Limits<T>::inf();
            const unsigned long long bu = __ballot(u), bb = __ballot(in && !u);
            if (lane == 0) { s_cnt[0][wave] = __popcll(bu); s_cnt[1][wave] = __popcll(bb); }
            __syncthreads();
            int offu = ubase, offb = bbase;
            for (int q = 0; q < wave; q++) { offu += s_cnt[0][q]; offb += s_cnt[1][q]; }
            const unsigned long long lt = (1ull << lane) - 1ull;
            if (u) perm[offu + __popcll(bu & lt)] = i;
            else if (in) perm[nu + offb + __popcll(bb & lt)] = i;
            for (int q = 0; q < WG / 64; q++) { ubase += s_cnt[0][q]; bbase += s_cnt[1][q]; }
            __syncthreads();
        }
    }
    for (int p = tid; p < m; p += WG) {
        const int i = perm[p];
        pb1[p] = jb[2 * i]; pb2[p] = jb[2 * i + 1];
        if (p >= nu) {
            lo[p - nu] = rows[(size_t)i * RW_COUNT + RW_LO]; hi[p - nu] = rows[(size_t)i * RW_COUNT + RW_HI];
            state[p - nu] = ST_FREE; lam[p - nu] = T(0);
        }
    }
    __syncthreads();
    // ---- A, permuted, packed lower, with the right-hand side as row m
    for (int p = tid; p <= m; p += WG) {
        T *Mp = M + tri(p, 0);
        if (p == m) { for (int q = 0; q < m; q++) Mp[q] = rows[(size_t)perm[q] * RW_COUNT + RW_RHS]; Mp[m] = T(0); continue; }
        const int i = perm[p], i1 = pb1[p], i2 = pb2[p];
        const T *ji = rows + (size_t)i * RW_COUNT + RW_J;
        for (int q = 0; q <= p; q++) {
            const int j1 = pb1[q], j2 = pb2[q];
            T a = T(0);
            if (i1 == j1 || i1 == j2 || (i2 >= 0 && (i2 == j1 || i2 == j2))) {
                const T *pj = rows + (size_t)perm[q] * RW_COUNT + RW_IMJ;
                if (i1 == j1) { for (int e = 0; e < 6; e++) a = fma_(ji[e], pj[e], a); }
                if (j2 >= 0 && i1 == j2) { for (int e = 0; e < 6; e++) a = fma_(ji[e], pj[6 + e], a); }
                if (i2 >= 0 && i2 == j1) { for (int e = 0; e < 6; e++) a = fma_(ji[6 + e], pj[e], a); }
                if (i2 >= 0 && j2 >= 0 && i2 == j2) { for (int e = 0; e < 6; e++) a = fma_(ji[6 + e], pj[6 + e], a); }
            }
            if (q == p) a += rows[(size_t)i * RW_COUNT + RW_AD];
            Mp[q] = a;
        }
    }
    __syncthreads();
    // ---- U eliminated: what is left in rows / columns nu.. is the Schur complement and the reduced right-hand side
    ldlt_steps<T, WG>(M, m, 0, nu, dinv, tol, tid);
    const int max_rounds = 20 * m + 100;
    (void)lds_pivot_rounds<T, WG>(M, m, nu, nbd, W, lam, wv, lo, hi, state, fidx, viol, z, tol, murty_only, max_rounds, tid);
    if constexpr (APX) {
        int has = 0;
        for (int q = tid; q < nbd; q += WG) has |= rows[(size_t)perm[nu + q] * RW_COUNT + RW_FMU] > T(0) ? 1 : 0;
        if (__syncthreads_or(has)) {
            // lambda^A of the bounded rows (the normal rows are among them) into the rows, clamped as the final store clamps
            for (int q = tid; q < nbd; q += WG) {
                T l = lam[q];
                if (state[q] == ST_FREE) { if (l < lo[q]) l = lo[q]; if (l > hi[q]) l = hi[q]; }
                rows[(size_t)perm[nu + q] * RW_COUNT + RW_LAM] = l;
            }
            __syncthreads();
            for (int q = tid; q < nbd; q += WG) {
                const int i = perm[nu + q];
                const T *row = rows + (size_t)i * RW_COUNT;
                const T fmu = row[RW_FMU];
                if (fmu > T(0)) pyramid_bounds(fmu, rows[(size_t)(i - (int)row[RW_FDIR]) * RW_COUNT + RW_LAM], lo[q], hi[q]);
                state[q] = ST_FREE; lam[q] = T(0);
            }
            __syncthreads();
            (void)lds_pivot_rounds<T, WG>(M, m, nu, nbd, W, lam, wv, lo, hi, state, fidx, viol, z, tol, murty_only, max_rounds, tid);
        }
    }
    // ---- lambda_U: L_UU^T x = D^-1 y_U - L_BU^T lambda_B
    for (int k = tid; k < nu; k += WG) {
        T acc = M[tri(m, k)];
        for (int e = 0; e < nbd; e++) acc = fma_(-M[tri(nu + e, k)], lam[e], acc);
        z[k] = acc * dinv[k];
    }
    __syncthreads();
    ldlt_backsub<T, WG>(M, nu, dinv, z, tid);
    // lambda into the rows (free rows clamped to their bounds as the oracle does), residual, forces, integration
    double resid = 0.0;
    for (int p = tid; p < m; p += WG) {
        const int i = perm[p];
        T l;
        if (p < nu) l = z[p];
        else {
            const int q = p - nu;
            l = lam[q];
            const T w = wv[q];
            if (state[q] == ST_FREE) { if (l < lo[q]) l = lo[q]; if (l > hi[q]) l = hi[q]; resid += (double)tabs(w); }
            else resid += (double)(state[q] == ST_LO ? (w < T(0) ? -w : T(0)) : (w > T(0) ? w : T(0)));
        }
        rows[(size_t)i * RW_COUNT + RW_LAM] = l;
    }
    __syncthreads();
    for (int k = tid; k < nb; k += WG) {
        T f[6] = { T(0), T(0), T(0), T(0), T(0), T(0) };
        for (int i = 0; i < m; i++) {
            const int2 bb = *reinterpret_cast<const int2 *>(jb + 2 * (size_t)i);
            if (bb.x != k && bb.y != k) continue;
            const T *ip = rows + (size_t)i * RW_COUNT + RW_IMJ;
            const T l = rows[(size_t)i * RW_COUNT + RW_LAM];
            if (bb.x == k) { for (int q = 0; q < 6; q++) f[q] = fma_(l, ip[q], f[q]); }
            if (bb.y == k) { for (int q = 0; q < 6; q++) f[q] = fma_(l, ip[6 + q], f[q]); }
        }
        T *b = bs + (size_t)k * BW_COUNT;
        for (int q = 0; q < 6; q++) b[BW_FC + q] = f[q];
        finish_body(S, bflags, stride, b, I.bodies[b0 + k], m > 0, h, I.damping);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) resid += __shfl_xor(resid, o, 64);
    if (lane == 0 && resid != 0.0) atomicAdd(&diag->residual, resid);
    if (tid == 0) atomicAdd(&diag->contacts, (unsigned long long)nc);
}

}  // namespace
}  // namespace dmx
