// damping_harness.cpp -- csrc/dmx_damping.hpp's damp_body and csrc/dmx_island_rows.hpp's finish_body with its angular speed cap on
// the host, in the precision chosen at compile time (-DROWS_SINGLE: float), as an evaluator for tests/test_damping_harness.py: the
// functions the damping pass and every integrator of the joints tick call per slot, fed from a slab of a few tiles.
//
//   damping_harness <cases.bin> <out.bin>
// cases.bin  two doubles (h, null_table: 1 = no table exists -- no damping pass, finish_body is handed a null pointer), then records
//            of 12 doubles, one per slot: lvel3 avel3 flags lin_scale ang_scale lin_threshold ang_threshold max_angular_speed
// out.bin    records of 14 doubles: lvel3 avel3 after damp_body; lvel3 avel3 after finish_body (no rows, no force, no torque, unit
//            mass and inertia: the velocity update adds zeros); 1 if the pose finish_body left is the one integrate_quat and the
//            position update give from the pre-tick pose with the velocities it left, else 0; 1 if it cleared the accumulators
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "dmx_island_rows.hpp"

#ifdef ROWS_SINGLE
typedef float real;
#else
typedef double real;
#endif
using namespace dmx;

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: damping_harness <cases.bin> <out.bin>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    double head[2];
    if (fread(head, sizeof(double), 2, f) != 2) { fprintf(stderr, "no header in %s\n", argv[1]); return 2; }
    std::vector<double> in;
    double rec[12];
    while (fread(rec, sizeof(double), 12, f) == 12) in.insert(in.end(), rec, rec + 12);
    fclose(f);
    const real h = (real)head[0];
    const bool null_table = head[1] != 0.0;
    const int n = (int)(in.size() / 12);
    const int stride = (n + SLAB_TILE - 1) / SLAB_TILE * SLAB_TILE;
    std::vector<real> S((size_t)C_COUNT * stride, real(0));
    std::vector<uint8_t> flags((size_t)stride, 0);
    std::vector<real> table((size_t)DAMP_REALS * stride, real(0));
    for (int s = 0; s < n; s++) {
        const double *r = in.data() + (size_t)12 * s;
        for (int c = 0; c < 6; c++) S[(size_t)slab_ix(C_LVEL + c, s)] = (real)r[c];
        // a pose that is no identity, and accumulators that finish_body must clear
        S[(size_t)slab_ix(C_POS + 0, s)] = real(0.25) * real(s); S[(size_t)slab_ix(C_POS + 1, s)] = real(1.5); S[(size_t)slab_ix(C_POS + 2, s)] = real(-0.75);
        Q4<real> q = { real(0.9), real(0.1) * real(s % 3), real(-0.2), real(0.3) };
        normalize(q);
        S[(size_t)slab_ix(C_QUAT + 0, s)] = q.w; S[(size_t)slab_ix(C_QUAT + 1, s)] = q.x; S[(size_t)slab_ix(C_QUAT + 2, s)] = q.y; S[(size_t)slab_ix(C_QUAT + 3, s)] = q.z;
        for (int c = 0; c < 6; c++) S[(size_t)slab_ix(C_FORCE + c, s)] = real(1 + c);
        flags[(size_t)s] = (uint8_t)r[6];
        for (int c = 0; c < DAMP_REALS; c++) table[(size_t)DAMP_REALS * s + c] = (real)r[7 + c];
    }
    real b[BW_COUNT];
    for (int c = 0; c < BW_COUNT; c++) b[c] = real(0);
    b[BW_INVI + 0] = b[BW_INVI + 4] = b[BW_INVI + 8] = real(1);
    b[BW_INVM] = real(1);
    FILE *o = fopen(argv[2], "wb");
    if (!o) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    for (int s = 0; s < n; s++) {
        double out[14];
        if (!null_table) damp_body<real>(S.data(), flags.data(), table.data(), s);
        for (int c = 0; c < 6; c++) out[c] = S[(size_t)slab_ix(C_LVEL + c, s)];
        V3<real> x = ldS(S.data(), (int64_t)stride, C_POS, s);
        Q4<real> q = { S[(size_t)slab_ix(C_QUAT + 0, s)], S[(size_t)slab_ix(C_QUAT + 1, s)], S[(size_t)slab_ix(C_QUAT + 2, s)], S[(size_t)slab_ix(C_QUAT + 3, s)] };
        finish_body<real>(S.data(), flags.data(), (int64_t)stride, b, s, false, h, null_table ? nullptr : table.data());
        for (int c = 0; c < 6; c++) out[6 + c] = S[(size_t)slab_ix(C_LVEL + c, s)];
        const V3<real> v = ldS(S.data(), (int64_t)stride, C_LVEL, s), w = ldS(S.data(), (int64_t)stride, C_AVEL, s);
        x.x = fma_(h, v.x, x.x); x.y = fma_(h, v.y, x.y); x.z = fma_(h, v.z, x.z);
        integrate_quat(q, w, h);
        const bool pose = x.x == S[(size_t)slab_ix(C_POS + 0, s)] && x.y == S[(size_t)slab_ix(C_POS + 1, s)] && x.z == S[(size_t)slab_ix(C_POS + 2, s)] &&
                          q.w == S[(size_t)slab_ix(C_QUAT + 0, s)] && q.x == S[(size_t)slab_ix(C_QUAT + 1, s)] && q.y == S[(size_t)slab_ix(C_QUAT + 2, s)] &&
                          q.z == S[(size_t)slab_ix(C_QUAT + 3, s)];
        bool cleared = true;
        for (int c = 0; c < 6; c++) cleared = cleared && S[(size_t)slab_ix(C_FORCE + c, s)] == real(0);
        out[12] = pose ? 1.0 : 0.0; out[13] = cleared ? 1.0 : 0.0;
        fwrite(out, sizeof(double), 14, o);
    }
    fclose(o);
    return 0;
}
