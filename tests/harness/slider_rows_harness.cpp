// slider_rows_harness.cpp -- csrc/dmx_island_rows.hpp's joint_unit_rows for the units of a slider and of a fixed joint, and
// slider_position, on the host, in the precision chosen at compile time (-DROWS_SINGLE: float), as an evaluator for
// tests/test_slider_reference.py: the functions the island kernels build these rows with, fed from a one-tile slab and from
// entries staged as csrc/dmx_joints.cpp stages them (a joint's units back to back).
//
//   slider_rows_harness <cases.bin> <out.bin>
// cases.bin  records of 48 doubles: kind (3 slider / 4 fixed), has body 2 (0 / 1), sides exchanged (0 / 1), limot present (0 / 1),
//            pos3 quat4 of body 1, pos3 quat4 of body 2 (of the ENTRY: after an exchange body 1 is the given body 2), anchor1 3,
//            anchor2 3, axis1 3 (all three of the entry's sides), axis1 as given 3, q_0c 4, lo_stop, hi_stop, vel, fmax, erp, h, cfm,
//            seven spares
// out.bin    records of 114 doubles: the row count, s (slider_position of the sides as given; 0 for a fixed joint), then per row
//            (seven slots) J[12], c, cfm, lo, hi
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
    if (argc != 3) { fprintf(stderr, "usage: slider_rows_harness <cases.bin> <out.bin>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::vector<double> in;
    double rec[48];
    while (fread(rec, sizeof(double), 48, f) == 48) in.insert(in.end(), rec, rec + 48);
    fclose(f);
    FILE *o = fopen(argv[2], "wb");
    if (!o) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    std::vector<real> S((size_t)C_COUNT * SLAB_TILE, real(0));
    for (size_t k = 0; k + 48 <= in.size(); k += 48) {
        const double *r = in.data() + k;
        const int kind = (int)r[0], two = (int)r[1], rev = (int)r[2], limot = (int)r[3];
        for (int b = 0; b < 2; b++) {
            for (int c = 0; c < 3; c++) S[(size_t)slab_ix(C_POS + c, b)] = (real)r[4 + 7 * b + c];
            for (int c = 0; c < 4; c++) S[(size_t)slab_ix(C_QUAT + c, b)] = (real)r[7 + 7 * b + c];
        }
        // up to three entries: slider = lock, linear, limot; fixed = ball, lock
        real cpos[9] = { 0 }, cnormal[9] = { 0 }, cdepth[3] = { 0 }, cmu[3] = { 0 }, s0[3] = { 0 }, s1[3] = { 0 }, s2[3] = { 0 }, s3[3] = { 0 };
        int cb1[3] = { 0, 0, 0 }, cb2[3], cmode[3] = { 0, 0, 0 }, local[2] = { 0, 1 };
        for (int e = 0; e < 3; e++) cb2[e] = two ? 1 : -1;
        int ne = 0;
        auto lock = [&](int e) {
            for (int c = 0; c < 3; c++) cnormal[3 * e + c] = (real)r[30 + c];
            cdepth[e] = (real)r[33]; cmu[e] = (real)UNIT_LOCK_MU;
        };
        auto anchors = [&](int e, double marker) {
            for (int c = 0; c < 3; c++) { cpos[3 * e + c] = (real)r[18 + c]; cnormal[3 * e + c] = (real)r[21 + c]; }
            cmu[e] = (real)marker;
        };
        if (kind == 3) {
            lock(0);
            anchors(1, UNIT_SLIDER2_MU);
            s0[1] = (real)r[24]; s1[1] = (real)r[25]; s2[1] = (real)r[26];
            ne = 2;
            if (limot) {
                for (int c = 0; c < 3; c++) cpos[6 + c] = (real)r[27 + c];
                cmu[2] = (real)UNIT_SLIMOT_MU; cmode[2] = rev;
                s0[2] = (real)r[34]; s1[2] = (real)r[35]; s2[2] = (real)r[36]; s3[2] = (real)r[37];
                ne = 3;
            }
        } else {
            anchors(0, UNIT_BALL_MU);
            lock(1);
            ne = 2;
        }
        IslandSet<real> I = {};
        I.cb1 = cb1; I.cb2 = cb2; I.cmode = cmode; I.local = local; I.cpos = cpos; I.cnormal = cnormal; I.cdepth = cdepth; I.cmu = cmu;
        I.cbounce = s0; I.cbounce_vel = s1; I.csoft_erp = s2; I.csoft_cfm = s3; I.has_units = 1;
        StepParams<real> P = {};
        P.erp = (real)r[38]; P.h = (real)r[39]; P.cfm = (real)r[40];
        real rows[9 * RW_COUNT] = { 0 };
        int jb[18] = { 0 };
        int m = 0;
        for (int e = 0; e < ne; e++) {
            const int n = joint_unit_rows<real>(S.data(), SLAB_TILE, I, P, rows, jb, e, m, real(1) / P.h);
            if (n != unit_rows_of(cmu[e])) { fprintf(stderr, "case %zu: entry %d gave %d rows\n", k / 48, e, n); return 1; }
            m += n;
        }
        for (int q = 0; q < m; q++)
            if (jb[2 * q] != 0 || jb[2 * q + 1] != (two ? 1 : -1)) { fprintf(stderr, "case %zu: row %d, bodies %d %d\n", k / 48, q, jb[2 * q], jb[2 * q + 1]); return 1; }
        double out[114] = { 0 };
        out[0] = m;
        if (kind == 3) {
            // the sides as given: after an exchange the given side 1 is the world, with the entry's second anchor
            const V3<real> zero = { real(0), real(0), real(0) };
            const V3<real> xa = { (real)r[4], (real)r[5], (real)r[6] }, xb = { (real)r[11], (real)r[12], (real)r[13] };
            const Q4<real> qa = { (real)r[7], (real)r[8], (real)r[9], (real)r[10] }, qb = { (real)r[14], (real)r[15], (real)r[16], (real)r[17] };
            const V3<real> an1 = { (real)r[18], (real)r[19], (real)r[20] }, an2 = { (real)r[21], (real)r[22], (real)r[23] };
            const V3<real> axis = { (real)r[27], (real)r[28], (real)r[29] };
            real s, sd;
            if (rev) slider_position<real>(false, zero, qa, zero, zero, true, xa, qa, zero, zero, an2, an1, axis, s, sd);
            else slider_position<real>(true, xa, qa, zero, zero, two != 0, xb, qb, zero, zero, an1, an2, axis, s, sd);
            out[1] = s;
        }
        for (int q = 0; q < m; q++) {
            const real *row = rows + (size_t)q * RW_COUNT;
            double *w = out + 2 + 16 * q;
            for (int j = 0; j < 12; j++) w[j] = row[RW_J + j];
            w[12] = row[RW_RHS]; w[13] = row[RW_AD]; w[14] = row[RW_LO]; w[15] = row[RW_HI];
        }
        fwrite(out, sizeof(double), 114, o);
    }
    fclose(o);
    return 0;
}
