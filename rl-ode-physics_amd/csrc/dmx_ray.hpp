// dmx_ray.hpp -- a ray against one geom: the primitives behind dmxBatchRayCast (dmx_raycast.hip, one call per candidate) and
// the ODE face's dCollide(ray, geom) (ode_compat.cpp, on the host).  Templates on the real type, host and device, every array
// index a compile-time constant (registers, no scratch memory), fused multiply-adds only where written (dot, mulv), like
// dmx_collide.hpp.
//
// Ray: the segment o + t d, 0 <= t <= len, d the given direction normalised in T.  Hit: the smallest t of the segment at which
// it crosses the geom's surface; the normal is the surface's outward unit normal there, negated when the origin lies inside the
// solid, so dot(normal, d) <= 0.  An origin exactly on the surface counts as outside.  [ODE-recall]: what ODE's ray colliders
// return (dCollideRaySphere / RayBox / RayPlane / RayConvex), restated from memory; see DESIGN.md section 5.
#pragma once

#include "dmx_math.hpp"

namespace dmx {

template <class T> struct Ray { V3<T> o, d; T len; };
template <class T> struct RayHit { T t; V3<T> n; };

template <class T> DMX_HD bool ray_finite(T x) { return x - x == T(0); }

// the caller's origin, direction and length -> a ray; false (a miss whatever the scene holds) when the direction's norm is zero
// or not finite or the length is not finite or <= 0
template <class T> DMX_HD bool ray_make(T ox, T oy, T oz, T dx, T dy, T dz, T len, Ray<T> &r)
{
    const T l2 = dx * dx + dy * dy + dz * dz;
    if (!(l2 > T(0)) || !ray_finite(l2) || !ray_finite(len) || !(len > T(0)) || !ray_finite(ox + oy + oz)) return false;
    const T l = tsqrt<T>(l2);
    r.o = { ox, oy, oz };
    r.d = { dx / l, dy / l, dz / l };
    r.len = len;
    return true;
}

// can the segment reach the sphere (c, rad) at all?  m = o - c.  Distance of the segment's nearest point, squared, against rad^2
template <class T> DMX_HD bool ray_misses_ball(const V3<T> &m, const Ray<T> &r, T rad)
{
    T tc = -dot(m, r.d);
    tc = tc < T(0) ? T(0) : (tc > r.len ? r.len : tc);
    const V3<T> q = { m.x + tc * r.d.x, m.y + tc * r.d.y, m.z + tc * r.d.z };
    return dot(q, q) > rad * rad;
}

// Sphere: the quadratic, written through the ray's foot point q = m - (m.d) d (the discriminant as rad^2 - |q|^2, not
// (m.d)^2 - (|m|^2 - rad^2), which cancels for distant origins).  Near root from outside, far root from inside.
template <class T> DMX_HD bool ray_sphere(const Ray<T> &r, const V3<T> &c, T rad, RayHit<T> &h)
{
    const V3<T> m = { r.o.x - c.x, r.o.y - c.y, r.o.z - c.z };
    const T b = dot(m, r.d);
    const V3<T> q = { m.x - b * r.d.x, m.y - b * r.d.y, m.z - b * r.d.z };
    const T disc = rad * rad - dot(q, q);
    if (!(disc >= T(0))) return false;
    const T s = tsqrt<T>(disc);
    const bool inside = dot(m, m) < rad * rad;
    const T t = inside ? s - b : -b - s;
    if (!(t >= T(0)) || !(t <= r.len)) return false;
    const T k = (inside ? T(-1) : T(1)) / rad;
    h.t = t;
    h.n = { (m.x + t * r.d.x) * k, (m.y + t * r.d.y) * k, (m.z + t * r.d.z) * k };
    return true;
}

// Box (centre c, rotation R body -> world, side lengths): slab test in the box frame; the normal is the axis of the crossed
// face (the entering face from outside, the leaving one from inside; the lowest axis on ties), turned against the ray
template <class T> DMX_HD bool ray_box(const Ray<T> &r, const V3<T> &c, const M3<T> &R, const V3<T> &side, RayHit<T> &h)
{
    const V3<T> m = { r.o.x - c.x, r.o.y - c.y, r.o.z - c.z };
    // R^T m, R^T d: the columns of R are the box's axes
    const T mo[3] = { fma_(R.m[2][0], m.z, fma_(R.m[1][0], m.y, R.m[0][0] * m.x)),
                      fma_(R.m[2][1], m.z, fma_(R.m[1][1], m.y, R.m[0][1] * m.x)),
                      fma_(R.m[2][2], m.z, fma_(R.m[1][2], m.y, R.m[0][2] * m.x)) };
    const T md[3] = { fma_(R.m[2][0], r.d.z, fma_(R.m[1][0], r.d.y, R.m[0][0] * r.d.x)),
                      fma_(R.m[2][1], r.d.z, fma_(R.m[1][1], r.d.y, R.m[0][1] * r.d.x)),
                      fma_(R.m[2][2], r.d.z, fma_(R.m[1][2], r.d.y, R.m[0][2] * r.d.x)) };
    const T hs[3] = { T(0.5) * side.x, T(0.5) * side.y, T(0.5) * side.z };
    T t_in = -Limits<T>::inf(), t_out = Limits<T>::inf();
    int a_in = 0, a_out = 0;
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        if (!(tabs(mo[a]) < hs[a])) inside = false;
        if (md[a] == T(0)) {
            if (tabs(mo[a]) > hs[a]) return false;
            continue;
        }
        T t1 = (-hs[a] - mo[a]) / md[a], t2 = (hs[a] - mo[a]) / md[a];
        if (t1 > t2) { const T u = t1; t1 = t2; t2 = u; }
        if (t1 > t_in) { t_in = t1; a_in = a; }
        if (t2 < t_out) { t_out = t2; a_out = a; }
    }
    if (!(t_in <= t_out)) return false;
    const T t = inside ? t_out : t_in;
    const int a = inside ? a_out : a_in;
    if (!(t >= T(0)) || !(t <= r.len)) return false;
    const T mda = a == 0 ? md[0] : (a == 1 ? md[1] : md[2]);
    const T sg = mda > T(0) ? T(-1) : T(1);
    h.t = t;
    h.n = { sg * (a == 0 ? R.m[0][0] : (a == 1 ? R.m[0][1] : R.m[0][2])),
            sg * (a == 0 ? R.m[1][0] : (a == 1 ? R.m[1][1] : R.m[1][2])),
            sg * (a == 0 ? R.m[2][0] : (a == 1 ? R.m[2][1] : R.m[2][2])) };
    return true;
}

// Plane n.x = d (n a unit vector): hit from either side, the normal faces the side the ray comes from
template <class T> DMX_HD bool ray_plane(const Ray<T> &r, const V3<T> &n, T d, RayHit<T> &h)
{
    const T so = dot(n, r.o) - d, dn = dot(n, r.d);
    if (dn == T(0)) return false;
    const T t = -so / dn;
    if (!(t >= T(0)) || !(t <= r.len)) return false;
    const T sg = dn > T(0) ? T(-1) : T(1);
    h.t = t;
    h.n = { sg * n.x, sg * n.y, sg * n.z };
    return true;
}

// Convex hull (centre c, rotation R, nf face planes (unit outward normal, offset) in the body frame, bounding radius rb): the
// bounding sphere first, then the segment clipped against the faces in the body frame: the latest entering face from outside,
// the earliest leaving face from inside; the first face in array order on ties
template <class T> DMX_HD bool ray_convex(const Ray<T> &r, const V3<T> &c, const M3<T> &R, const T *planes, int nf, T rb, RayHit<T> &h)
{
    const V3<T> m = { r.o.x - c.x, r.o.y - c.y, r.o.z - c.z };
    if (nf <= 0 || ray_misses_ball(m, r, rb)) return false;
    const V3<T> mo = { fma_(R.m[2][0], m.z, fma_(R.m[1][0], m.y, R.m[0][0] * m.x)),
                       fma_(R.m[2][1], m.z, fma_(R.m[1][1], m.y, R.m[0][1] * m.x)),
                       fma_(R.m[2][2], m.z, fma_(R.m[1][2], m.y, R.m[0][2] * m.x)) };
    const V3<T> md = { fma_(R.m[2][0], r.d.z, fma_(R.m[1][0], r.d.y, R.m[0][0] * r.d.x)),
                       fma_(R.m[2][1], r.d.z, fma_(R.m[1][1], r.d.y, R.m[0][1] * r.d.x)),
                       fma_(R.m[2][2], r.d.z, fma_(R.m[1][2], r.d.y, R.m[0][2] * r.d.x)) };
    T t_in = -Limits<T>::inf(), t_out = Limits<T>::inf();
    V3<T> n_in = { T(0), T(0), T(0) }, n_out = { T(0), T(0), T(0) };
    bool inside = true;
    for (int f = 0; f < nf; f++) {
        const V3<T> n = { planes[4 * f], planes[4 * f + 1], planes[4 * f + 2] };
        const T dist = dot(n, mo) - planes[4 * f + 3], dn = dot(n, md);
        if (!(dist < T(0))) inside = false;
        if (dn == T(0)) {
            if (dist > T(0)) return false;
            continue;
        }
        const T t = -dist / dn;
        if (dn < T(0)) { if (t > t_in) { t_in = t; n_in = n; } }
        else if (t < t_out) { t_out = t; n_out = n; }
    }
    if (!(t_in <= t_out)) return false;
    const T t = inside ? t_out : t_in;
    if (!(t >= T(0)) || !(t <= r.len)) return false;
    const V3<T> nb = inside ? V3<T>{ -n_out.x, -n_out.y, -n_out.z } : n_in;
    h.t = t;
    h.n = mulv(R, nb);
    return true;
}

// ---- the walk of a ray's (x,z) projection through a grid of square columns (dmx_raycast.hip; host and device, so that a host
// harness can hold it against brute force) ----------------------------------------------------------------------------------
// the columns' width and the (x,z) rectangle of the centres of everything a ray can see
template <class T> struct RayGrid { T cell, inv_cell, xmin, xmax, zmin, zmax; };

DMX_HD int ray_cell(double v)
{
    return (int)__builtin_floor(v < -2.0e9 ? -2.0e9 : (v > 2.0e9 ? 2.0e9 : v));
}

// The walk.  visit(cx, cz, ax, az): test the buckets of the three columns (cx + k ax, cz + k az), k = -1, 0, 1;  bound(): the
// best t so far (what a strip further along the ray can no longer beat).  The walk covers the part of the segment inside the
// visible bodies' rectangle, widened by a column (no body reaches further out than its bounding radius, < half a column): a
// ray of length 1e9 costs what that part costs.  Column boundaries are recomputed from the column index at every step (no
// running sum, whose rounding would grow with the step count); what rounding is left -- which of two columns a point within
// an ulp of their boundary counts to -- is covered by the dilation, which has 0.6 columns to spare.
template <class T, class V, class B>
DMX_HD void ray_walk(const RayGrid<T> &Sc, const Ray<T> &ray, V visit, B bound)
{
    const T x0 = Sc.xmin - Sc.cell, x1 = Sc.xmax + Sc.cell;
    const T z0 = Sc.zmin - Sc.cell, z1 = Sc.zmax + Sc.cell;
    if (!(x0 <= x1) || !(z0 <= z1)) return;                 // nobody to see (or the rectangle is not a number)
    T ta = T(0), tb = ray.len;
    if (ray.d.x != T(0)) {
        T t1 = (x0 - ray.o.x) / ray.d.x, t2 = (x1 - ray.o.x) / ray.d.x;
        if (t1 > t2) { const T u = t1; t1 = t2; t2 = u; }
        ta = t1 > ta ? t1 : ta; tb = t2 < tb ? t2 : tb;
    } else if (ray.o.x < x0 || ray.o.x > x1) return;
    if (ray.d.z != T(0)) {
        T t1 = (z0 - ray.o.z) / ray.d.z, t2 = (z1 - ray.o.z) / ray.d.z;
        if (t1 > t2) { const T u = t1; t1 = t2; t2 = u; }
        ta = t1 > ta ? t1 : ta; tb = t2 < tb ? t2 : tb;
    } else if (ray.o.z < z0 || ray.o.z > z1) return;
    if (!(ta <= tb)) return;
    int ix = ray_cell((double)((ray.o.x + ta * ray.d.x) * Sc.inv_cell)), iz = ray_cell((double)((ray.o.z + ta * ray.d.z) * Sc.inv_cell));
    const int sx = ray.d.x > T(0) ? 1 : -1, sz = ray.d.z > T(0) ? 1 : -1;
    // no walk crosses more columns than the rectangle has, both ways together
    const double span = ((double)(x1 - x0) + (double)(z1 - z0)) * (double)Sc.inv_cell + 8.0;
    int guard = span < 6.7e7 ? (int)span : 67108864;
    for (int k = -1; k <= 1; k++) visit(ix + k, iz, 0, 1);
    while (guard-- > 0) {
        // a vertical ray, or one along a grid axis: no boundary of that direction is ever crossed
        const T tx = ray.d.x != T(0) ? ((T)(ix + (sx > 0 ? 1 : 0)) * Sc.cell - ray.o.x) / ray.d.x : Limits<T>::inf();
        const T tz = ray.d.z != T(0) ? ((T)(iz + (sz > 0 ? 1 : 0)) * Sc.cell - ray.o.z) / ray.d.z : Limits<T>::inf();
        const bool step_x = tx <= tz;
        const T tn = step_x ? tx : tz;
        if (!(tn <= tb) || tn > bound() + Sc.cell) break;
        if (step_x) { ix += sx; visit(ix + sx, iz, 0, 1); }
        else { iz += sz; visit(ix, iz + sz, 1, 0); }
    }
}

}  // namespace dmx
