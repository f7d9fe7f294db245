// ray_prims_harness.cpp -- csrc/dmx_ray.hpp on the host, in the precision chosen at compile time (-DRAY_SINGLE: float), as an
// evaluator for tests/test_ray_reference.py: reads ray-geom pairs, writes what the primitives return.
//
//   ray_prims_harness <pairs.bin> <planes.bin> <out.bin>
//   ray_prims_harness walk <xbits> <spheres.bin> <rays.bin> <out.bin>
// The second form holds the grid walk (ray_walk, what the device's lane and wavefront forms run) against brute force on the
// host: spheres (4 doubles each: centre3, radius) are binned by cell_hash into a 1 024-bucket table exactly as bp_insert bins
// bodies (torus of 2^xbits columns, or scrambled for xbits = 0); per ray (7 doubles) out.bin gets 5 doubles: the walk's best t
// (-1: none) and sphere, brute force's, and the number of candidates the walk tested.
// pairs.bin   records of 18 doubles: class (1 sphere, 2 box, 3 convex, 4 plane), origin3, direction3, length, centre3 (plane: its
//             unit normal), quaternion4 (w, x, y, z), sides3 (sphere: radius; convex: bounding radius; plane: offset) -- values
//             of the harness's precision
// planes.bin  the hull's faces, 4 doubles each (may be empty)
// out.bin     records of 6 doubles: ray valid, hit, t, normal3
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include <string.h>
#include "dmx_grid.hpp"
#include "dmx_ray.hpp"

#ifdef RAY_SINGLE
typedef float real;
#else
typedef double real;
#endif
using namespace dmx;

static std::vector<double> slurp(const char *path)
{
    std::vector<double> v;
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", path); exit(2); }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    v.resize((size_t)bytes / sizeof(double));
    if (!v.empty() && fread(v.data(), sizeof(double), v.size(), f) != v.size()) { fprintf(stderr, "short read of %s\n", path); exit(2); }
    fclose(f);
    return v;
}

static int walk_mode(int xbits, const char *spheres_path, const char *rays_path, const char *out_path)
{
    const std::vector<double> sp = slurp(spheres_path), rays = slurp(rays_path);
    const size_t n = sp.size() / 4, nr = rays.size() / 7;
    double rmax = 0;
    for (size_t i = 0; i < n; i++) rmax = sp[4 * i + 3] > rmax ? sp[4 * i + 3] : rmax;
    RayGrid<real> G;
    G.cell = (real)(2.0 * 1.25 * rmax); G.inv_cell = real(1) / G.cell;
    G.xmin = G.zmin = Limits<real>::inf(); G.xmax = G.zmax = -Limits<real>::inf();
    const uint32_t mask = 1023u;
    std::vector<std::vector<int>> bucket(mask + 1);
    for (size_t i = 0; i < n; i++) {
        const real x = (real)sp[4 * i], z = (real)sp[4 * i + 2];
        bucket[cell_hash((int)floor((double)(x * G.inv_cell)), (int)floor((double)(z * G.inv_cell)), mask, xbits)].push_back((int)i);
        G.xmin = x < G.xmin ? x : G.xmin; G.xmax = x > G.xmax ? x : G.xmax;
        G.zmin = z < G.zmin ? z : G.zmin; G.zmax = z > G.zmax ? z : G.zmax;
    }
    std::vector<double> out(nr * 5, -1.0);
    for (size_t k = 0; k < nr; k++) {
        const double *r = &rays[7 * k];
        Ray<real> ray;
        if (!ray_make<real>((real)r[0], (real)r[1], (real)r[2], (real)r[3], (real)r[4], (real)r[5], (real)r[6], ray)) continue;
        real best_t[2] = { Limits<real>::inf(), Limits<real>::inf() };
        int best_i[2] = { -1, -1 };
        long tested = 0;
        auto test = [&](int i, int w) {
            const V3<real> c = { (real)sp[4 * i], (real)sp[4 * i + 1], (real)sp[4 * i + 2] };
            const V3<real> m = { ray.o.x - c.x, ray.o.y - c.y, ray.o.z - c.z };
            RayHit<real> h;
            if (ray_misses_ball<real>(m, ray, (real)sp[4 * i + 3]) || !ray_sphere<real>(ray, c, (real)sp[4 * i + 3], h)) return;
            if (h.t < best_t[w] || (h.t == best_t[w] && i < best_i[w])) { best_t[w] = h.t; best_i[w] = i; }
        };
        ray_walk<real>(G, ray, [&](int cx, int cz, int ax, int az) {
            for (int q = -1; q <= 1; q++)
                for (int i : bucket[cell_hash(cx + q * ax, cz + q * az, mask, xbits)]) { test(i, 0); tested++; }
        }, [&]() { return best_t[0]; });
        for (size_t i = 0; i < n; i++) test((int)i, 1);
        double *o = &out[5 * k];
        o[0] = best_i[0] < 0 ? -1.0 : (double)best_t[0]; o[1] = best_i[0];
        o[2] = best_i[1] < 0 ? -1.0 : (double)best_t[1]; o[3] = best_i[1];
        o[4] = (double)tested;
    }
    FILE *f = fopen(out_path, "wb");
    if (!f || fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) { fprintf(stderr, "cannot write %s\n", out_path); return 2; }
    fclose(f);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 6 && !strcmp(argv[1], "walk")) return walk_mode(atoi(argv[2]), argv[3], argv[4], argv[5]);
    if (argc != 4) { fprintf(stderr, "usage: %s pairs.bin planes.bin out.bin\n", argv[0]); return 2; }
    const std::vector<double> in = slurp(argv[1]), pl = slurp(argv[2]);
    std::vector<real> planes(pl.begin(), pl.end());
    const int nf = (int)(planes.size() / 4);
    const size_t n = in.size() / 18;
    std::vector<double> out(n * 6, 0.0);
    for (size_t k = 0; k < n; k++) {
        const double *r = &in[18 * k];
        double *o = &out[6 * k];
        Ray<real> ray;
        if (!ray_make<real>((real)r[1], (real)r[2], (real)r[3], (real)r[4], (real)r[5], (real)r[6], (real)r[7], ray)) continue;
        o[0] = 1.0;
        const V3<real> c = { (real)r[8], (real)r[9], (real)r[10] };
        const M3<real> R = quat_to_R(Q4<real>{ (real)r[11], (real)r[12], (real)r[13], (real)r[14] });
        RayHit<real> h = { 0, { 0, 0, 0 } };
        bool hit = false;
        switch ((int)r[0]) {
        case 1: hit = ray_sphere<real>(ray, c, (real)r[15], h); break;
        case 2: hit = ray_box<real>(ray, c, R, V3<real>{ (real)r[15], (real)r[16], (real)r[17] }, h); break;
        case 3: hit = ray_convex<real>(ray, c, R, planes.data(), nf, (real)r[15], h); break;
        case 4: hit = ray_plane<real>(ray, c, (real)r[15], h); break;
        default: fprintf(stderr, "record %zu: unknown class\n", k); return 2;
        }
        if (hit) { o[1] = 1.0; o[2] = (double)h.t; o[3] = (double)h.n.x; o[4] = (double)h.n.y; o[5] = (double)h.n.z; }
    }
    FILE *f = fopen(argv[3], "wb");
    if (!f || fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) { fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
    fclose(f);
    return 0;
}
