// friction_sweep_harness.cpp -- the island kernels' own phase functions (csrc/dmx_island_rows.hpp: stage_body, contact_rows, body_tmp,
// row_setup, row_sor, finish_body) run on the host over whole small islands, in the instantiations a tick with pyramid rows
// (DMX_CONTACT_APPROX1) launches, in the precision chosen at compile time (-DROWS_SINGLE: float): QuickStep's sweeps in creation
// order as solve_islands_body makes them.  An evaluator for tests/test_friction_harness.py.
//
//   friction_sweep_harness <cases.bin> <out.bin>
// cases.bin  per island: a header of 10 doubles (bodies nb, contacts nc, h, erp, cfm, sor_w, iters, gravity 3), nb records of 17
//            doubles (pos3 quat4 lvel3 avel3 mass inertia3) and nc records of 15 doubles in canonical form (pos3 normal3 depth,
//            body1, body2 or -1 as indices into the island's bodies, mode, mu, bounce, bounce_vel, soft_erp, soft_cfm)
// out.bin    per island: the row count m, lambda[m], then 6 doubles per body: its linear and angular velocity after the tick
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
    if (argc != 3) { fprintf(stderr, "usage: friction_sweep_harness <cases.bin> <out.bin>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    FILE *o = fopen(argv[2], "wb");
    if (!o) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    double head[10];
    std::vector<real> S((size_t)C_COUNT * SLAB_TILE, real(0));
    std::vector<uint8_t> bflags((size_t)SLAB_TILE, (uint8_t)BF_ALIVE);
    while (fread(head, sizeof(double), 10, f) == 10) {
        const int nb = (int)head[0], nc = (int)head[1];
        if (nb < 1 || nb > 16 || nc < 0 || nc > 64) { fprintf(stderr, "bad island: %d bodies, %d contacts\n", nb, nc); return 1; }
        StepParams<real> P = {};
        P.h = (real)head[2]; P.erp = (real)head[3]; P.cfm = (real)head[4]; P.sor_w = (real)head[5]; P.iters = (int)head[6];
        P.g = { (real)head[7], (real)head[8], (real)head[9] };
        for (int b = 0; b < nb; b++) {
            double r[17];
            if (fread(r, sizeof(double), 17, f) != 17) return 1;
            for (int c = 0; c < 3; c++) {
                S[(size_t)slab_ix(C_POS + c, b)] = (real)r[c]; S[(size_t)slab_ix(C_LVEL + c, b)] = (real)r[7 + c];
                S[(size_t)slab_ix(C_AVEL + c, b)] = (real)r[10 + c]; S[(size_t)slab_ix(C_INERTIA + c, b)] = (real)r[14 + c];
                S[(size_t)slab_ix(C_FORCE + c, b)] = real(0); S[(size_t)slab_ix(C_TORQUE + c, b)] = real(0);
            }
            for (int c = 0; c < 4; c++) S[(size_t)slab_ix(C_QUAT + c, b)] = (real)r[3 + c];
            S[(size_t)slab_ix(C_MASS, b)] = (real)r[13];
        }
        std::vector<real> cpos(3 * (size_t)nc + 1), cnormal(3 * (size_t)nc + 1), cdepth(nc + 1), cmu(nc + 1), cbounce(nc + 1), cbv(nc + 1), cserp(nc + 1), cscfm(nc + 1);
        std::vector<int> cb1(nc + 1), cb2(nc + 1), cmode(nc + 1), local(SLAB_TILE, 0);
        for (int c = 0; c < nc; c++) {
            double r[15];
            if (fread(r, sizeof(double), 15, f) != 15) return 1;
            for (int k = 0; k < 3; k++) { cpos[3 * (size_t)c + k] = (real)r[k]; cnormal[3 * (size_t)c + k] = (real)r[3 + k]; }
            cdepth[c] = (real)r[6]; cb1[c] = (int)r[7]; cb2[c] = (int)r[8]; cmode[c] = (int)r[9]; cmu[c] = (real)r[10];
            cbounce[c] = (real)r[11]; cbv[c] = (real)r[12]; cserp[c] = (real)r[13]; cscfm[c] = (real)r[14];
        }
        IslandSet<real> I = {};
        I.n_islands = 1;
        I.cb1 = cb1.data(); I.cb2 = cb2.data(); I.cmode = cmode.data(); I.local = local.data();
        I.cpos = cpos.data(); I.cnormal = cnormal.data(); I.cdepth = cdepth.data(); I.cmu = cmu.data();
        I.cbounce = cbounce.data(); I.cbounce_vel = cbv.data(); I.csoft_erp = cserp.data(); I.csoft_cfm = cscfm.data();
        // solve_islands_body<real, true, true>, island 0, bodies 0 .. nb - 1
        const real h = P.h, hinv = real(1) / h;
        std::vector<real> bs((size_t)nb * BW_COUNT), rows((size_t)(3 * nc + 1) * RW_COUNT, real(0));
        std::vector<int> jb(2 * (size_t)(3 * nc + 1));
        for (int k = 0; k < nb; k++) stage_body(S.data(), bflags.data(), (int64_t)SLAB_TILE, I, P, bs.data() + (size_t)k * BW_COUNT, k, k);
        int m = 0;
        for (int c = 0; c < nc; c++) {
            contact_rows<real, 0, true>(S.data(), (int64_t)SLAB_TILE, I, P, rows.data(), jb.data(), c, m, hinv);
            m += cmu[c] > 0 ? 3 : 1;
        }
        if (m > 0) {
            for (int k = 0; k < nb; k++) body_tmp(S.data(), (int64_t)SLAB_TILE, bs.data() + (size_t)k * BW_COUNT, k, hinv);
            for (int i = 0; i < m; i++) row_setup<real, true, true>(rows.data(), jb.data(), bs.data(), i, hinv, P.sor_w);
            for (int it = 0; it < P.iters; it++)
                for (int i = 0; i < m; i++) (void)row_sor<real, true>(rows.data(), jb.data(), bs.data(), i);
        }
        for (int k = 0; k < nb; k++) finish_body(S.data(), bflags.data(), (int64_t)SLAB_TILE, bs.data() + (size_t)k * BW_COUNT, k, m > 0, h);
        std::vector<double> out;
        out.push_back((double)m);
        for (int i = 0; i < m; i++) out.push_back((double)rows[(size_t)i * RW_COUNT + RW_LAM]);
        for (int k = 0; k < nb; k++) {
            for (int c = 0; c < 3; c++) out.push_back((double)S[(size_t)slab_ix(C_LVEL + c, k)]);
            for (int c = 0; c < 3; c++) out.push_back((double)S[(size_t)slab_ix(C_AVEL + c, k)]);
        }
        fwrite(out.data(), sizeof(double), out.size(), o);
    }
    fclose(f);
    fclose(o);
    return 0;
}
