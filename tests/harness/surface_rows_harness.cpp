// surface_rows_harness.cpp -- contact_rows<T, 0, true> (csrc/dmx_island_rows.hpp), the row builder of a tick whose contacts carry more
// than box friction, run on the host over single contacts with the extended surface staged behind them (IslandSet::cext), in the
// precision chosen at compile time (-DROWS_SINGLE: float).  An evaluator for tests/test_surface_harness.py.
//
//   surface_rows_harness <cases.bin> <out.bin>
// cases.bin  per contact: a header of 4 doubles (h, erp, cfm, 1 = with the extension / 0 = the pointer is null), two bodies of 9
//            doubles (pos3 lvel3 avel3), the contact in canonical form, 15 doubles (pos3 normal3 depth, body1, body2 or -1, mode as
//            staged, mu as staged, bounce, bounce_vel, soft_erp, soft_cfm), and the EXT_REALS staged reals
// out.bin    per contact: the row count, then per row 18 doubles: J[12], lo, hi, c, cfm, RW_FMU, RW_FDIR; then one double: with the
//            pointer null, the number of reals among J, c, cfm, lo, hi in which the rows differ, bit for bit, from those of
//            contact_rows<T, 0, false> -- compared only for a contact without DMX_CONTACT_APPROX1 bits -- else 0
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
    if (argc != 3) { fprintf(stderr, "usage: surface_rows_harness <cases.bin> <out.bin>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    FILE *o = fopen(argv[2], "wb");
    if (!o) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    double head[4];
    std::vector<real> S((size_t)C_COUNT * SLAB_TILE, real(0));
    while (fread(head, sizeof(double), 4, f) == 4) {
        StepParams<real> P = {};
        P.h = (real)head[0]; P.erp = (real)head[1]; P.cfm = (real)head[2];
        const bool with_ext = head[3] != 0.0;
        for (int b = 0; b < 2; b++) {
            double r[9];
            if (fread(r, sizeof(double), 9, f) != 9) return 1;
            for (int c = 0; c < 3; c++) {
                S[(size_t)slab_ix(C_POS + c, b)] = (real)r[c]; S[(size_t)slab_ix(C_LVEL + c, b)] = (real)r[3 + c];
                S[(size_t)slab_ix(C_AVEL + c, b)] = (real)r[6 + c];
            }
        }
        double r[15], e[EXT_REALS];
        if (fread(r, sizeof(double), 15, f) != 15 || fread(e, sizeof(double), EXT_REALS, f) != (size_t)EXT_REALS) return 1;
        real cpos[3], cnormal[3], cdepth = (real)r[6], cmu = (real)r[10], cbounce = (real)r[11], cbv = (real)r[12], cserp = (real)r[13], cscfm = (real)r[14];
        real cext[EXT_REALS];
        for (int k = 0; k < 3; k++) { cpos[k] = (real)r[k]; cnormal[k] = (real)r[3 + k]; }
        for (int k = 0; k < EXT_REALS; k++) cext[k] = (real)e[k];
        int cb1 = (int)r[7], cb2 = (int)r[8], cmode = (int)r[9];
        std::vector<int> local(SLAB_TILE, 0);
        local[1] = 1;
        IslandSet<real> I = {};
        I.n_islands = 1;
        I.cb1 = &cb1; I.cb2 = &cb2; I.cmode = &cmode; I.local = local.data();
        I.cpos = cpos; I.cnormal = cnormal; I.cdepth = &cdepth; I.cmu = &cmu;
        I.cbounce = &cbounce; I.cbounce_vel = &cbv; I.csoft_erp = &cserp; I.csoft_cfm = &cscfm;
        I.cext = with_ext ? cext : nullptr;
        const real hinv = real(1) / P.h;
        real rows[4 * RW_COUNT], plain[4 * RW_COUNT];
        int jb[8], jbp[8];
        memset(rows, 0, sizeof rows); memset(plain, 0, sizeof plain);
        contact_rows<real, 0, true>(S.data(), (int64_t)SLAB_TILE, I, P, rows, jb, 0, 0, hinv);
        const int rpc = cmu > 0 ? 3 : 1;
        double differ = 0.0;
        if (!with_ext && !(cmode & SURF_APPROX1)) {
            contact_rows<real, 0, false>(S.data(), (int64_t)SLAB_TILE, I, P, plain, jbp, 0, 0, hinv);
            const int fields[5] = { RW_RHS, RW_AD, RW_LO, RW_HI, RW_LAM };
            for (int i = 0; i < rpc; i++) {
                for (int j = 0; j < 12; j++) differ += memcmp(&rows[i * RW_COUNT + RW_J + j], &plain[i * RW_COUNT + RW_J + j], sizeof(real)) ? 1.0 : 0.0;
                for (int q = 0; q < 5; q++) differ += memcmp(&rows[i * RW_COUNT + fields[q]], &plain[i * RW_COUNT + fields[q]], sizeof(real)) ? 1.0 : 0.0;
                differ += (jb[2 * i] != jbp[2 * i] || jb[2 * i + 1] != jbp[2 * i + 1]) ? 1.0 : 0.0;
            }
        }
        std::vector<double> out;
        out.push_back((double)rpc);
        for (int i = 0; i < rpc; i++) {
            const real *row = rows + (size_t)i * RW_COUNT;
            for (int j = 0; j < 12; j++) out.push_back((double)row[RW_J + j]);
            out.push_back((double)row[RW_LO]); out.push_back((double)row[RW_HI]); out.push_back((double)row[RW_RHS]);
            out.push_back((double)row[RW_AD]); out.push_back((double)row[RW_FMU]); out.push_back((double)row[RW_FDIR]);
        }
        out.push_back(differ);
        fwrite(out.data(), sizeof(double), out.size(), o);
    }
    fclose(f);
    fclose(o);
    return 0;
}
