// dmx_raycast.hip -- batched ray casts against the scene (dmxBatchRayCast): per ray the first geom its segment crosses, where,
// and with which normal (dmx_ray.hpp holds the ray-geom primitives; DESIGN.md "Ray casts" the reasoning).
//
// Three forms of one computation -- same candidates' tests, same winner rule, same bits:
//   lane   a lane per ray walks the ray's (x,z) projection through the hashed column grid (dmx_grid.hpp; buckets filled by
//          bp_insert into a table of the ray cast's own), dilated by one column each way: a body sits in its centre's column
//          only and a column is at least 1.25 bounding diameters wide, so the body a ray point touches has its centre at most
//          one column away.  For 10^4 .. 10^6 rays.
//   wave   a wavefront per ray: the same walk, wave-uniform, a strip's candidates numbered across its buckets and dealt to the
//          64 lanes (ex_pair_count_wave's pattern), the best (t, rank) by a wave reduction.  For a handful of rays into a pen.
//   brute  a lane per ray tests every slot: the on-device cross-check and timing baseline, never chosen automatically.
// The winner is the smallest t; ties go to the lowest rank (plane, static boxes in order, bodies by slot), so the answer does
// not depend on the order candidates come up in -- or on how often: a bucket shared across a torus period, or met by two
// strips of a scrambled table, only repeats tests.
// Index work and a few dozen flops per candidate: bound by the dependent L2 round trips of the walk (count -> items -> the
// candidate's centre and radius), which the strip's three buckets issue together.  Hull faces are read from device memory (the
// teapot's 2 526 faces, 40 KiB in f32, do not fit beside the static boxes in a budget that keeps 8 waves per SIMD; the loads are
// wave-uniform when the lanes of a wave test the same face index, and L2-resident); static boxes sit in LDS.
#include <hip/hip_runtime.h>
#include "dmx_internal.hpp"
#include "dmx_math.hpp"
#include "dmx_grid.hpp"
#include "dmx_ray.hpp"

namespace dmx {

constexpr uint32_t RAY_RANK_PLANE = 0u, RAY_RANK_STATIC = 1u, RAY_RANK_BODY = 1u + (uint32_t)MAX_STATIC_BOXES, RAY_RANK_NONE = 0xffffffffu;

template <class T> struct RayBest { T t; uint32_t rank; V3<T> n; };
template <class T> __device__ __forceinline__ void ray_take(RayBest<T> &b, const RayHit<T> &h, uint32_t rank)
{
    if (h.t < b.t || (h.t == b.t && rank < b.rank)) { b.t = h.t; b.rank = rank; b.n = h.n; }
}

// ---- the visible bodies' (x,z) bounding rectangle: one reduction per grid build ---------------------------------------------
// doubles as unsigned keys of the same order, for atomicMin / atomicMax
__device__ __forceinline__ unsigned long long ray_key(double x)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | (1ull << 63));
}
__device__ __forceinline__ double ray_unkey(unsigned long long k)
{
    return __longlong_as_double((long long)((k >> 63) ? (k & ~(1ull << 63)) : ~k));
}
__global__ void ray_bounds_init(unsigned long long *rect)
{
    if (threadIdx.x < 4) rect[threadIdx.x] = ray_key((threadIdx.x & 1) ? -__builtin_huge_val() : __builtin_huge_val());
}
template <class T>
__global__ __launch_bounds__(256) void ray_bounds(const T *__restrict__ S, const uint8_t *__restrict__ gtype, const uint8_t *__restrict__ bflags,
                                                  int64_t n, unsigned long long *__restrict__ rect)
{
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    double lo[2] = { __builtin_huge_val(), __builtin_huge_val() }, hi[2] = { -__builtin_huge_val(), -__builtin_huge_val() };
    if (i < n && gtype[i] != GEOM_NONE && (bflags[i] & BF_ALIVE)) {
        const double x = (double)S[slab_ix(C_POS + 0, i)], z = (double)S[slab_ix(C_POS + 2, i)];
        if (x == x) { lo[0] = x; hi[0] = x; }
        if (z == z) { lo[1] = z; hi[1] = z; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int a = 0; a < 2; a++) {
            const double l = __shfl_xor(lo[a], off, 64), h = __shfl_xor(hi[a], off, 64);
            lo[a] = l < lo[a] ? l : lo[a];
            hi[a] = h > hi[a] ? h : hi[a];
        }
    }
    if ((threadIdx.x & 63) == 0 && lo[0] <= hi[0]) {
        atomicMin(&rect[0], ray_key(lo[0])); atomicMax(&rect[1], ray_key(hi[0]));
        atomicMin(&rect[2], ray_key(lo[1])); atomicMax(&rect[3], ray_key(hi[1]));
    }
}

// ---- one candidate --------------------------------------------------------------------------------------------------------------
template <class T> __device__ __forceinline__ bool ray_sees(const RaySceneParams<T> &Sc, int gt, int64_t j)
{
    return gt != GEOM_NONE && gt <= GEOM_CONVEX && (Sc.bflags[j] & BF_ALIVE) && ((Sc.mask >> (gt - 1)) & 1u);
}
// slot j against the ray.  GRID: the candidate comes from a bucket -- its bounding radius is in the slab (C_BPR, left there by
// bp_insert; the value bound_radius gives), and the bounding sphere is tested before anything else is loaded.
template <class T, bool GRID>
__device__ __forceinline__ void ray_body(const RaySceneParams<T> &Sc, const Ray<T> &ray, int64_t j, RayBest<T> &best)
{
    const T *S = Sc.S;
    int gt = 0;
    T rb;
    if (GRID) rb = S[slab_ix(C_BPR, j)];
    else {
        gt = Sc.gtype[j];
        if (!ray_sees<T>(Sc, gt, j)) return;
        rb = bound_radius<T>(gt, S, j);
    }
    const V3<T> c = { S[slab_ix(C_POS + 0, j)], S[slab_ix(C_POS + 1, j)], S[slab_ix(C_POS + 2, j)] };
    const V3<T> m = { ray.o.x - c.x, ray.o.y - c.y, ray.o.z - c.z };
    if (ray_misses_ball<T>(m, ray, rb)) return;
    if (GRID) {
        gt = Sc.gtype[j];
        if (!ray_sees<T>(Sc, gt, j)) return;
    }
    RayHit<T> h;
    bool hit;
    if (gt == GEOM_SPHERE) hit = ray_sphere<T>(ray, c, S[slab_ix(C_SIDES + 0, j)], h);
    else {
        const M3<T> R = quat_to_R(Q4<T>{ S[slab_ix(C_QUAT + 0, j)], S[slab_ix(C_QUAT + 1, j)], S[slab_ix(C_QUAT + 2, j)], S[slab_ix(C_QUAT + 3, j)] });
        if (gt == GEOM_BOX)
            hit = ray_box<T>(ray, c, R, V3<T>{ S[slab_ix(C_SIDES + 0, j)], S[slab_ix(C_SIDES + 1, j)], S[slab_ix(C_SIDES + 2, j)] }, h);
        else
            hit = ray_convex<T>(ray, c, R, Sc.hull_planes, Sc.hull_nf, S[slab_ix(C_SIDES + 0, j)], h);
    }
    if (hit) ray_take<T>(best, h, RAY_RANK_BODY + (uint32_t)j);
}

template <class T> __device__ __forceinline__ void ray_static(const RaySceneParams<T> &Sc, const T *sb, const Ray<T> &ray, int s, RayBest<T> &best)
{
    const T *b = sb + s * SBOX_REALS;
    M3<T> R;
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int c = 0; c < 3; c++) R.m[a][c] = b[SBOX_R + 3 * a + c];
    RayHit<T> h;
    if (ray_box<T>(ray, V3<T>{ b[SBOX_POS], b[SBOX_POS + 1], b[SBOX_POS + 2] }, R, V3<T>{ b[SBOX_SIDE], b[SBOX_SIDE + 1], b[SBOX_SIDE + 2] }, h))
        ray_take<T>(best, h, RAY_RANK_STATIC + (uint32_t)s);
}
template <class T> __device__ __forceinline__ void ray_ground(const RaySceneParams<T> &Sc, const Ray<T> &ray, RayBest<T> &best)
{
    RayHit<T> h;
    if (Sc.plane_on && (Sc.mask & DMX_RAYMASK_PLANE) && ray_plane<T>(ray, Sc.pn, Sc.pd, h)) ray_take<T>(best, h, RAY_RANK_PLANE);
}

// the static boxes into LDS (every thread of the block calls this, before anything can return)
template <class T> __device__ __forceinline__ void ray_stage_statics(const RaySceneParams<T> &Sc, T *sb)
{
    for (int k = threadIdx.x; k < Sc.n_static * SBOX_REALS; k += blockDim.x) sb[k] = Sc.sbox[k];
    __syncthreads();
}

template <class T> __device__ __forceinline__ bool ray_load(const T *__restrict__ rays, int64_t i, Ray<T> &ray)
{
    const T *r = rays + 7 * i;
    return ray_make<T>(r[0], r[1], r[2], r[3], r[4], r[5], r[6], ray);
}
template <class T>
__device__ __forceinline__ void ray_store(int64_t i, bool valid, const Ray<T> &ray, const RayBest<T> &best, int32_t *__restrict__ ids, T *__restrict__ hits)
{
    T *o = hits + 7 * i;
    if (!valid) {
        ids[i] = DMX_RAYID_MISS;
#pragma unroll
        for (int k = 0; k < 7; k++) o[k] = T(0);
        return;
    }
    const bool hit = best.rank != RAY_RANK_NONE;
    const T t = hit ? best.t : ray.len;
    ids[i] = !hit ? DMX_RAYID_MISS : best.rank == RAY_RANK_PLANE ? DMX_RAYID_PLANE
           : best.rank < RAY_RANK_BODY ? -3 - (int32_t)(best.rank - RAY_RANK_STATIC) : (int32_t)(best.rank - RAY_RANK_BODY);
    o[0] = ray.o.x + t * ray.d.x; o[1] = ray.o.y + t * ray.d.y; o[2] = ray.o.z + t * ray.d.z;
    o[3] = hit ? best.n.x : T(0); o[4] = hit ? best.n.y : T(0); o[5] = hit ? best.n.z : T(0);
    o[6] = t;
}

template <class T> __device__ __forceinline__ RayGrid<T> ray_grid(const RaySceneParams<T> &Sc)
{
    return { Sc.cell, Sc.inv_cell, (T)ray_unkey(Sc.rect[0]), (T)ray_unkey(Sc.rect[1]), (T)ray_unkey(Sc.rect[2]), (T)ray_unkey(Sc.rect[3]) };
}

// ---- lane per ray ----------------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void ray_cast_lane(RaySceneParams<T> Sc, int64_t n_rays, const T *__restrict__ rays,
                                                     int32_t *__restrict__ ids, T *__restrict__ hits)
{
    __shared__ T sb[MAX_STATIC_BOXES * SBOX_REALS];
    ray_stage_statics<T>(Sc, sb);
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n_rays) return;
    Ray<T> ray;
    RayBest<T> best = { Limits<T>::inf(), RAY_RANK_NONE, { T(0), T(0), T(0) } };
    const bool valid = ray_load<T>(rays, i, ray);
    if (valid) {
        ray_ground<T>(Sc, ray, best);
        if (Sc.mask & DMX_RAYMASK_STATIC)
            for (int s = 0; s < Sc.n_static; s++) ray_static<T>(Sc, sb, ray, s, best);
        if (Sc.mask & DMX_RAYMASK_BODIES)
            ray_walk<T>(ray_grid<T>(Sc), ray, [&](int cx, int cz, int ax, int az) {
                // the strip's three buckets: counts and first items fetched together, ahead of the tests
                uint32_t h[3], cnt[3];
                int4 it[3];
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    h[k] = cell_hash(cx + (k - 1) * ax, cz + (k - 1) * az, Sc.gmask, Sc.xbits);
                    cnt[k] = Sc.count[h[k]];
                    it[k] = *reinterpret_cast<const int4 *>(Sc.items + (size_t)h[k] * Sc.cap);
                }
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const uint32_t c = cnt[k] > (uint32_t)Sc.cap ? (uint32_t)Sc.cap : cnt[k];
                    for (uint32_t s = 0; s < c; s++) {
                        const int32_t j = s == 0 ? it[k].x : (s == 1 ? it[k].y : (s == 2 ? it[k].z : (s == 3 ? it[k].w
                                        : Sc.items[(size_t)h[k] * Sc.cap + s])));
                        ray_body<T, true>(Sc, ray, j, best);
                    }
                }
            }, [&]() { return best.t; });
    }
    ray_store<T>(i, valid, ray, best, ids, hits);
}

// ---- wavefront per ray -----------------------------------------------------------------------------------------------------------
template <class T> __device__ __forceinline__ T ray_wave_min(T v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { const T o = __shfl_xor(v, off, 64); v = o < v ? o : v; }
    return v;
}
template <class T>
__global__ __launch_bounds__(256) void ray_cast_wave(RaySceneParams<T> Sc, int64_t n_rays, const T *__restrict__ rays,
                                                     int32_t *__restrict__ ids, T *__restrict__ hits)
{
    __shared__ T sb[MAX_STATIC_BOXES * SBOX_REALS];
    ray_stage_statics<T>(Sc, sb);
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);          // wave-uniform
    if (i >= n_rays) return;
    Ray<T> ray;
    RayBest<T> best = { Limits<T>::inf(), RAY_RANK_NONE, { T(0), T(0), T(0) } };
    const bool valid = ray_load<T>(rays, i, ray);                             // every lane loads the same seven reals
    if (valid) {
        if (lane == 0) ray_ground<T>(Sc, ray, best);
        if ((Sc.mask & DMX_RAYMASK_STATIC) && lane < Sc.n_static) ray_static<T>(Sc, sb, ray, lane, best);
        T wave_best = ray_wave_min<T>(best.t);
        if (Sc.mask & DMX_RAYMASK_BODIES)
            ray_walk<T>(ray_grid<T>(Sc), ray, [&](int cx, int cz, int ax, int az) {
                // lanes 0..2: their column's bucket and its count; everyone: the running totals; then a lane per candidate
                uint32_t myh = 0, mycnt = 0;
                if (lane < 3) {
                    myh = cell_hash(cx + (lane - 1) * ax, cz + (lane - 1) * az, Sc.gmask, Sc.xbits);
                    mycnt = Sc.count[myh];
                    if (mycnt > (uint32_t)Sc.cap) mycnt = (uint32_t)Sc.cap;
                }
                const uint32_t h0 = __shfl(myh, 0, 64), h1 = __shfl(myh, 1, 64), h2 = __shfl(myh, 2, 64);
                const uint32_t e0 = __shfl(mycnt, 0, 64), e1 = e0 + __shfl(mycnt, 1, 64), e2 = e1 + __shfl(mycnt, 2, 64);
                for (uint32_t u = lane; u < e2; u += 64) {
                    const uint32_t hb = u < e0 ? h0 : (u < e1 ? h1 : h2), s = u < e0 ? u : (u < e1 ? u - e0 : u - e1);
                    ray_body<T, true>(Sc, ray, Sc.items[(size_t)hb * Sc.cap + s], best);
                }
                wave_best = ray_wave_min<T>(best.t);
            }, [&]() { return wave_best; });
        // the wave's winner: smallest (t, rank); its normal from the first lane that holds it
        T t = best.t; uint32_t rank = best.rank;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const T ot = __shfl_xor(t, off, 64); const uint32_t orank = __shfl_xor(rank, off, 64);
            if (ot < t || (ot == t && orank < rank)) { t = ot; rank = orank; }
        }
        const unsigned long long holders = __ballot(best.t == t && best.rank == rank);
        const int src = holders ? __ffsll((long long)holders) - 1 : 0;
        best.n.x = __shfl(best.n.x, src, 64); best.n.y = __shfl(best.n.y, src, 64); best.n.z = __shfl(best.n.z, src, 64);
        best.t = t; best.rank = rank;
    }
    if (lane == 0) ray_store<T>(i, valid, ray, best, ids, hits);
}

// ---- brute: every ray against every slot ---------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void ray_cast_brute(RaySceneParams<T> Sc, int64_t n_rays, const T *__restrict__ rays,
                                                      int32_t *__restrict__ ids, T *__restrict__ hits)
{
    __shared__ T sb[MAX_STATIC_BOXES * SBOX_REALS];
    ray_stage_statics<T>(Sc, sb);
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= n_rays) return;
    Ray<T> ray;
    RayBest<T> best = { Limits<T>::inf(), RAY_RANK_NONE, { T(0), T(0), T(0) } };
    const bool valid = ray_load<T>(rays, i, ray);
    if (valid) {
        ray_ground<T>(Sc, ray, best);
        if (Sc.mask & DMX_RAYMASK_STATIC)
            for (int s = 0; s < Sc.n_static; s++) ray_static<T>(Sc, sb, ray, s, best);
        if (Sc.mask & DMX_RAYMASK_BODIES)
            for (int64_t j = 0; j < Sc.n; j++) ray_body<T, false>(Sc, ray, j, best);
    }
    ray_store<T>(i, valid, ray, best, ids, hits);
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------
template <class T>
hipError_t launch_ray_bounds(const T *S, const uint8_t *gtype, const uint8_t *bflags, int64_t n, unsigned long long *rect, hipStream_t st)
{
    hipLaunchKernelGGL(ray_bounds_init, dim3(1), dim3(64), 0, st, rect);
    if (n > 0) hipLaunchKernelGGL((ray_bounds<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, S, gtype, bflags, n, rect);
    return hipGetLastError();
}
template <class T>
hipError_t launch_ray_cast(int form, const RaySceneParams<T> &Sc, int64_t n_rays, const T *rays, int32_t *ids, T *hits, hipStream_t st)
{
    if (n_rays <= 0) return hipSuccess;
    if (form == RAY_FORM_WAVE)
        hipLaunchKernelGGL((ray_cast_wave<T>), dim3((unsigned)((n_rays + 3) / 4)), dim3(256), 0, st, Sc, n_rays, rays, ids, hits);
    else if (form == RAY_FORM_BRUTE)
        hipLaunchKernelGGL((ray_cast_brute<T>), dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, st, Sc, n_rays, rays, ids, hits);
    else
        hipLaunchKernelGGL((ray_cast_lane<T>), dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, st, Sc, n_rays, rays, ids, hits);
    return hipGetLastError();
}
#define DMX_RAY_INST(T)                                                                                                           \
    template hipError_t launch_ray_bounds<T>(const T *, const uint8_t *, const uint8_t *, int64_t, unsigned long long *, hipStream_t); \
    template hipError_t launch_ray_cast<T>(int, const RaySceneParams<T> &, int64_t, const T *, int32_t *, T *, hipStream_t);
DMX_RAY_INST(float)
DMX_RAY_INST(double)

// the unit's code object and its kernels' first-use set-up, at dmxBatchCreate (see dmx_touch_broadphase)
hipError_t dmx_touch_raycast(int real_bytes)
{
    hipFuncAttributes a;
    hipError_t e = hipSuccess;
    auto touch = [&](const void *k) { const hipError_t r = hipFuncGetAttributes(&a, k); if (r != hipSuccess) e = r; };
    touch((const void *)&ray_bounds_init);
    if (real_bytes == 4) {
        touch((const void *)&ray_bounds<float>); touch((const void *)&ray_cast_lane<float>); touch((const void *)&ray_cast_wave<float>);
    } else {
        touch((const void *)&ray_bounds<double>); touch((const void *)&ray_cast_lane<double>); touch((const void *)&ray_cast_wave<double>);
    }
    return e;
}

}  // namespace dmx
