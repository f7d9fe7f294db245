// amotor_rows_harness.cpp -- csrc/dmx_amotor.hpp's amotor_axes and csrc/dmx_island_rows.hpp's joint_unit_rows for an angular motor's
// unit, on the host, in the precision chosen at compile time (-DROWS_SINGLE: float), as an evaluator for tests/test_amotor_harness.py:
// the function the prepare kernel calls and the builder the island kernels call, fed as the batch's tick feeds them.
//
//   amotor_rows_harness <cases.bin> <out.bin>
// cases.bin  records of 56 doubles: side 1 is a body (0 / 1), side 2 is a body (0 / 1) -- the sides AS GIVEN --, quat4 of side 1, quat4
//            of side 2, mode, num_axes, rel 3, axis 9, ref1 3, ref2 3, angle 3, lo_stop 3, hi_stop 3, vel 3, fmax 3, erp, h, cfm, the
//            axis whose row is built, spares
// out.bin    records of 28 doubles: a_0, a_1, a_2 (9), theta (3), then the row of that axis in the ENTRY's sides (given as (world,
//            body): exchanged): J[12], c, cfm, lo, hi
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "dmx_amotor.hpp"
#include "dmx_island_rows.hpp"

#ifdef ROWS_SINGLE
typedef float real;
#else
typedef double real;
#endif
using namespace dmx;

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: amotor_rows_harness <cases.bin> <out.bin>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::vector<double> in;
    double rec[56];
    while (fread(rec, sizeof(double), 56, f) == 56) in.insert(in.end(), rec, rec + 56);
    fclose(f);
    FILE *o = fopen(argv[2], "wb");
    if (!o) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    std::vector<real> S((size_t)C_COUNT * SLAB_TILE, real(0));
    for (size_t k = 0; k + 56 <= in.size(); k += 56) {
        const double *r = in.data() + k;
        const bool has1 = r[0] != 0, has2 = r[1] != 0;
        dmxAMotor m;
        memset(&m, 0, sizeof(m));
        m.mode = (int)r[10]; m.num_axes = (int)r[11];
        for (int i = 0; i < 3; i++) {
            m.rel[i] = (int)r[12 + i];
            for (int c = 0; c < 3; c++) m.axis[i][c] = r[15 + 3 * i + c];
            m.ref1[i] = r[24 + i]; m.ref2[i] = r[27 + i]; m.angle[i] = r[30 + i];
            m.lo_stop[i] = r[33 + i]; m.hi_stop[i] = r[36 + i]; m.vel[i] = r[39 + i]; m.fmax[i] = r[42 + i];
        }
        const int axis = (int)r[48];
        // what the batch holds: the quaternions in its precision (slot 0: side 1's body, slot 1: side 2's)
        for (int b = 0; b < 2; b++)
            for (int c = 0; c < 4; c++) S[(size_t)slab_ix(C_QUAT + c, b)] = (real)r[2 + 4 * b + c];
        // amotor_prepare's lane
        V3<real> a[3];
        real th[3];
        const Q4<real> ident = { real(1), real(0), real(0), real(0) };
        const real erp = (real)r[45], h = (real)r[46];
        real prep[AMOTOR_PREP_REALS];
        amotor_prepare_joint<real>(has1, has1 ? ldq(S.data(), 0) : ident, has2, has2 ? ldq(S.data(), 1) : ident, m, (real(1) / h) * erp, prep, a);
        for (int i = 0; i < 3; i++) th[i] = prep[AMOTOR_AXIS_REALS * i + AMP_THETA];
        // the entry as the tick stages it: (world, body) exchanges the sides
        const bool rev = !has1;
        int cb1[1] = { rev ? 1 : 0 }, cb2[1] = { rev ? -1 : (has2 ? 1 : -1) }, cmode[1] = { ((AMOTOR_AXIS_REALS * axis) << 1) | (rev ? 1 : 0) }, local[2] = { 0, 1 };
        real cmu[1] = { (real)UNIT_AMOTOR_MU };
        real lo_stop[1] = { 0 }, hi_stop[1] = { 0 }, vel[1] = { 0 }, fmax[1] = { 0 };      /* the four surface slots: zero, and not read */
        IslandSet<real> I = {};
        I.cb1 = cb1; I.cb2 = cb2; I.cmode = cmode; I.local = local; I.cmu = cmu;
        I.cbounce = lo_stop; I.cbounce_vel = hi_stop; I.csoft_erp = vel; I.csoft_cfm = fmax; I.has_units = 1;
        I.amotor = prep;
        StepParams<real> P = {};
        P.erp = (real)r[45]; P.h = (real)r[46]; P.cfm = (real)r[47];
        real rows[3 * RW_COUNT] = { 0 };
        int jb[6] = { 0 };
        const int n = joint_unit_rows<real>(S.data(), SLAB_TILE, I, P, rows, jb, 0, 0, real(1) / P.h);
        if (n != 1 || unit_rows_of(cmu[0]) != 1 || jb[0] != cb1[0] || jb[1] != cb2[0]) {
            fprintf(stderr, "case %zu: %d rows, bodies %d %d\n", k / 56, n, jb[0], jb[1]);
            return 1;
        }
        double out[28] = { 0 };
        for (int i = 0; i < 3; i++) { out[3 * i] = a[i].x; out[3 * i + 1] = a[i].y; out[3 * i + 2] = a[i].z; out[9 + i] = th[i]; }
        for (int j = 0; j < 12; j++) out[12 + j] = rows[RW_J + j];
        out[24] = rows[RW_RHS]; out[25] = rows[RW_AD]; out[26] = rows[RW_LO]; out[27] = rows[RW_HI];
        fwrite(out, sizeof(double), 28, o);
    }
    fclose(o);
    return 0;
}
