// joint_rows_harness.cpp -- csrc/dmx_island_rows.hpp's joint_unit_rows on the host, in the precision chosen at compile time
// (-DROWS_SINGLE: float), as an evaluator for tests/test_joint_reference.py: the function the island kernels call to make the rows
// of a ball / hinge joint's units, fed from a one-tile slab.
//
//   joint_rows_harness <cases.bin> <out.bin>
// cases.bin  records of 26 doubles: unit (1 ball, 2 hinge's angular rows), has body 2 (0 / 1), pos3 quat4 of body 1, pos3 quat4 of
//            body 2, the unit's six reals (first side 3, second side 3), erp, h, cfm, one spare
// out.bin    records of 1 + 3 x 16 doubles: the row count, then per row J[12], c, cfm, lo, hi (rows the unit does not have: zeros)
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
    if (argc != 3) { fprintf(stderr, "usage: joint_rows_harness <cases.bin> <out.bin>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::vector<double> in;
    double rec[26];
    while (fread(rec, sizeof(double), 26, f) == 26) in.insert(in.end(), rec, rec + 26);
    fclose(f);
    FILE *o = fopen(argv[2], "wb");
    if (!o) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    std::vector<real> S((size_t)C_COUNT * SLAB_TILE, real(0));
    for (size_t k = 0; k + 26 <= in.size(); k += 26) {
        const double *r = in.data() + k;
        const int unit = (int)r[0], two = (int)r[1];
        for (int b = 0; b < 2; b++) {
            for (int c = 0; c < 3; c++) S[(size_t)slab_ix(C_POS + c, b)] = (real)r[2 + 7 * b + c];
            for (int c = 0; c < 4; c++) S[(size_t)slab_ix(C_QUAT + c, b)] = (real)r[5 + 7 * b + c];
        }
        real cpos[3], cnormal[3], cmu[1] = { (real)(unit == UNIT_BALL ? UNIT_BALL_MU : UNIT_HINGE2_MU) };
        for (int c = 0; c < 3; c++) { cpos[c] = (real)r[16 + c]; cnormal[c] = (real)r[19 + c]; }
        int cb1[1] = { 0 }, cb2[1] = { two ? 1 : -1 }, local[2] = { 0, 1 };
        IslandSet<real> I = {};
        I.cb1 = cb1; I.cb2 = cb2; I.local = local; I.cpos = cpos; I.cnormal = cnormal; I.cmu = cmu; I.has_units = 1;
        StepParams<real> P = {};
        P.erp = (real)r[22]; P.h = (real)r[23]; P.cfm = (real)r[24];
        real rows[3 * RW_COUNT] = { 0 };
        int jb[6] = { 0 };
        const int n = joint_unit_rows<real>(S.data(), SLAB_TILE, I, P, rows, jb, 0, 0, real(1) / P.h);
        double out[1 + 3 * 16] = { 0 };
        out[0] = n;
        for (int q = 0; q < n; q++) {
            if (jb[2 * q] != 0 || jb[2 * q + 1] != (two ? 1 : -1)) { fprintf(stderr, "row %d: bodies %d %d\n", q, jb[2 * q], jb[2 * q + 1]); return 1; }
            const real *row = rows + (size_t)q * RW_COUNT;
            for (int j = 0; j < 12; j++) out[1 + 16 * q + j] = row[RW_J + j];
            out[1 + 16 * q + 12] = row[RW_RHS]; out[1 + 16 * q + 13] = row[RW_AD];
            out[1 + 16 * q + 14] = row[RW_LO]; out[1 + 16 * q + 15] = row[RW_HI];
        }
        fwrite(out, sizeof(double), 1 + 3 * 16, o);
    }
    fclose(o);
    return 0;
}
