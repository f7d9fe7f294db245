// feedback_rows_harness.cpp -- csrc/dmx_island_rows.hpp's joint_feedback / entry_feedback on the host, in the precision chosen at
// compile time (-DROWS_SINGLE: float), as an evaluator for tests/test_feedback_reference.py: the units of a slider or of a fixed
// joint are built by joint_unit_rows (as tests/harness/slider_rows_harness.cpp builds them), taken through row_setup in QuickStep's
// scaled form with feedback on and in dWorldStep's unscaled form, given prescribed multipliers, and handed to joint_feedback.
// Both forms must report J^T lambda of the rows as built.
//
//   feedback_rows_harness <cases.bin> <out.bin>
// cases.bin  records of 80 doubles: [0, 48) as slider_rows_harness's (kind, has body 2, sides exchanged, limot present, the two
//            bodies' pos3 quat4, anchors, axes, q_0c, lo_stop, hi_stop, vel, fmax, erp, h, cfm, ...); then for body 1 and body 2 the
//            inverse mass and the world inverse inertia (1 + 9 each, all zero for a kinematic body) at [49, 59) and [59, 69); seven
//            multipliers at [69, 76); sor_w at [76]
// out.bin    records of 116 doubles: the row count; the feedback from the scaled rows (12: f1 t1 f2 t2 in the sides as given); the
//            feedback from the unscaled rows (12); the rows' J as built (7 x 12); the factor the scaled form stored per row (7)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
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
    if (argc != 3) { fprintf(stderr, "usage: feedback_rows_harness <cases.bin> <out.bin>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::vector<double> in;
    double rec[80];
    while (fread(rec, sizeof(double), 80, f) == 80) in.insert(in.end(), rec, rec + 80);
    fclose(f);
    FILE *o = fopen(argv[2], "wb");
    if (!o) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    std::vector<real> S((size_t)C_COUNT * SLAB_TILE, real(0));
    for (size_t k = 0; k + 80 <= in.size(); k += 80) {
        const double *r = in.data() + k;
        const int kind = (int)r[0], two = (int)r[1], rev = (int)r[2], limot = (int)r[3];
        for (int b = 0; b < 2; b++) {
            for (int c = 0; c < 3; c++) S[(size_t)slab_ix(C_POS + c, b)] = (real)r[4 + 7 * b + c];
            for (int c = 0; c < 4; c++) S[(size_t)slab_ix(C_QUAT + c, b)] = (real)r[7 + 7 * b + c];
        }
        // up to three entries: slider = lock, linear, limot; fixed = ball, lock
        real cpos[9] = { 0 }, cnormal[9] = { 0 }, cdepth[3] = { 0 }, cmu[3] = { 0 }, s0[3] = { 0 }, s1[3] = { 0 }, s2[3] = { 0 }, s3[3] = { 0 };
        int cb1[3] = { 0, 0, 0 }, cb2[3], cmode[3] = { 0, 0, 0 }, local[2] = { 0, 1 }, crow[3] = { 0, 0, 0 };
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
        I.cbounce = s0; I.cbounce_vel = s1; I.csoft_erp = s2; I.csoft_cfm = s3; I.has_units = 1; I.crow = crow;
        StepParams<real> P = {};
        P.erp = (real)r[38]; P.h = (real)r[39]; P.cfm = (real)r[40];
        const real hinv = real(1) / P.h, sor_w = (real)r[76];
        real built[7 * RW_COUNT] = { 0 };
        int jb[14] = { 0 };
        int m = 0;
        for (int e = 0; e < ne; e++) {
            crow[e] = m;
            m += joint_unit_rows<real>(S.data(), SLAB_TILE, I, P, built, jb, e, m, hinv);
        }
        if (m > 7) { fprintf(stderr, "case %zu: %d rows\n", k / 80, m); return 1; }
        // the two bodies' scratch: inverse mass and inertia as given, v/h + M^-1 f = 0 (it reaches the right-hand side only)
        real bs[2 * BW_COUNT] = { 0 };
        for (int b = 0; b < 2; b++) {
            bs[b * BW_COUNT + BW_INVM] = (real)r[49 + 10 * b];
            for (int c = 0; c < 9; c++) bs[b * BW_COUNT + BW_INVI + c] = (real)r[50 + 10 * b + c];
        }
        real scaled[7 * RW_COUNT], plain[7 * RW_COUNT];
        memcpy(scaled, built, sizeof(built));
        memcpy(plain, built, sizeof(built));
        for (int q = 0; q < m; q++) {
            row_setup<real, true, true>(scaled, jb, bs, q, hinv, sor_w);
            row_setup<real, false>(plain, jb, bs, q, hinv, sor_w);
            scaled[(size_t)q * RW_COUNT + RW_LAM] = plain[(size_t)q * RW_COUNT + RW_LAM] = (real)r[69 + q];
        }
        real fa[12], fb[12];
        const int info = 2 * ne + (rev ? 1 : 0);
        joint_feedback<real>(I, P, scaled, 0, info, true, fa);
        joint_feedback<real>(I, P, plain, 0, info, false, fb);
        double out[116] = { 0 };
        out[0] = m;
        for (int j = 0; j < 12; j++) { out[1 + j] = fa[j]; out[13 + j] = fb[j]; }
        for (int q = 0; q < m; q++) {
            for (int j = 0; j < 12; j++) out[25 + 12 * q + j] = built[(size_t)q * RW_COUNT + RW_J + j];
            out[109 + q] = scaled[(size_t)q * RW_COUNT + RW_UNSCALE];
        }
        fwrite(out, sizeof(double), 116, o);
    }
    fclose(o);
    return 0;
}
