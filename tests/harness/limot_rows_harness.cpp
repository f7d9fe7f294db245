// limot_rows_harness.cpp -- csrc/dmx_island_rows.hpp's joint_unit_rows for a hinge's limit / motor unit, and hinge_angle, on the
// host, in the precision chosen at compile time (-DROWS_SINGLE: float), as an evaluator for tests/test_limot_reference.py: the
// functions the island kernels build the limot row with, fed from a one-tile slab.
//
//   limot_rows_harness <cases.bin> <out.bin>
// cases.bin  records of 32 doubles: has body 2 (0 / 1), sides exchanged (0 / 1), pos3 quat4 of body 1, pos3 quat4 of body 2 (of the
//            ENTRY: after an exchange body 1 is the given body 2), axis1 as given 3, q_0 4, lo_stop, hi_stop, vel, fmax, erp, h, cfm,
//            two spares
// out.bin    records of 18 doubles: the row count, theta (hinge_angle of the sides as given), J[12], c, cfm, lo, hi
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
    if (argc != 3) { fprintf(stderr, "usage: limot_rows_harness <cases.bin> <out.bin>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::vector<double> in;
    double rec[32];
    while (fread(rec, sizeof(double), 32, f) == 32) in.insert(in.end(), rec, rec + 32);
    fclose(f);
    FILE *o = fopen(argv[2], "wb");
    if (!o) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    std::vector<real> S((size_t)C_COUNT * SLAB_TILE, real(0));
    for (size_t k = 0; k + 32 <= in.size(); k += 32) {
        const double *r = in.data() + k;
        const int two = (int)r[0], rev = (int)r[1];
        for (int b = 0; b < 2; b++) {
            for (int c = 0; c < 3; c++) S[(size_t)slab_ix(C_POS + c, b)] = (real)r[2 + 7 * b + c];
            for (int c = 0; c < 4; c++) S[(size_t)slab_ix(C_QUAT + c, b)] = (real)r[5 + 7 * b + c];
        }
        real cpos[3], cnormal[3], cdepth[1], cmu[1] = { (real)UNIT_LIMOT_MU };
        for (int c = 0; c < 3; c++) { cpos[c] = (real)r[16 + c]; cnormal[c] = (real)r[19 + c]; }
        cdepth[0] = (real)r[22];
        real lo_stop[1] = { (real)r[23] }, hi_stop[1] = { (real)r[24] }, vel[1] = { (real)r[25] }, fmax[1] = { (real)r[26] };
        int cb1[1] = { 0 }, cb2[1] = { two ? 1 : -1 }, cmode[1] = { rev }, local[2] = { 0, 1 };
        IslandSet<real> I = {};
        I.cb1 = cb1; I.cb2 = cb2; I.cmode = cmode; I.local = local; I.cpos = cpos; I.cnormal = cnormal; I.cdepth = cdepth; I.cmu = cmu;
        I.cbounce = lo_stop; I.cbounce_vel = hi_stop; I.csoft_erp = vel; I.csoft_cfm = fmax; I.has_units = 1;
        StepParams<real> P = {};
        P.erp = (real)r[27]; P.h = (real)r[28]; P.cfm = (real)r[29];
        real rows[3 * RW_COUNT] = { 0 };
        int jb[6] = { 0 };
        const int n = joint_unit_rows<real>(S.data(), SLAB_TILE, I, P, rows, jb, 0, 0, real(1) / P.h);
        if (n != 1 || jb[0] != 0 || jb[1] != (two ? 1 : -1)) { fprintf(stderr, "case %zu: %d rows, bodies %d %d\n", k / 32, n, jb[0], jb[1]); return 1; }
        const Q4<real> ident = { real(1), real(0), real(0), real(0) };
        const Q4<real> qa = { (real)r[5], (real)r[6], (real)r[7], (real)r[8] }, qb = { (real)r[12], (real)r[13], (real)r[14], (real)r[15] };
        const Q4<real> q0 = { cnormal[0], cnormal[1], cnormal[2], cdepth[0] };
        const V3<real> axis1 = { cpos[0], cpos[1], cpos[2] };
        double out[18] = { 0 };
        out[0] = n;
        out[1] = rev ? hinge_angle(ident, qa, q0, axis1) : hinge_angle(qa, two ? qb : ident, q0, axis1);
        for (int j = 0; j < 12; j++) out[2 + j] = rows[RW_J + j];
        out[14] = rows[RW_RHS]; out[15] = rows[RW_AD]; out[16] = rows[RW_LO]; out[17] = rows[RW_HI];
        fwrite(out, sizeof(double), 18, o);
    }
    fclose(o);
    return 0;
}
