// single_contact_harness.cpp -- "contact_rows with the second body absent", executable: single_contact / single_contact_row
// (csrc/dmx_island_rows.hpp: what the one-lane island forms solve_singles_body and solve_singles_lds_body build their rows with) against
// contact_rows<T> itself with cb2 = -1, on the host, over seeded one-body contacts in float and in double.  Every row's J[0..6), c, cfm
// and bounds must carry the same bits as RW_J[0..6), RW_RHS, RW_AD, RW_LO and RW_HI of the row contact_rows writes, and the row
// counts must agree.  The population's coverage is counted and required here, and printed for the wrapper
// (tests/test_single_contact_harness.py).
//
//   single_contact_harness [contacts per precision, default 4096]
// exit status 0: every row equal and every class of the population met; 1 otherwise (the first differences are printed)
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "dmx_island_rows.hpp"

using namespace dmx;

struct Rng {        // xorshift64*: the same population wherever this is compiled
    uint64_t s;
    uint64_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return s * 2685821657736338717ull; }
    double uni(double lo, double hi) { return lo + (hi - lo) * (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
    int pick(int n) { return (int)(next() >> 33) % n; }
};

enum { COV_DIRECT, COV_INDIRECT, COV_LAUNCH_SURFACE, COV_OWN_SURFACE, COV_MU_ZERO, COV_MU_FINITE, COV_MU_INF, COV_SOFT_ERP_ON, COV_SOFT_ERP_OFF,
       COV_SOFT_CFM_ON, COV_SOFT_CFM_OFF, COV_BOUNCE_OFF, COV_BOUNCE_TAKEN, COV_BOUNCE_BELOW_VEL, COV_LAYER_ZERO, COV_LAYER_ABOVE_DEPTH,
       COV_MAXCORR_INF, COV_MAXCORR_BINDS, COV_NEGATIVE_DEPTH, COV_COUNT };
static const char *const cov_name[COV_COUNT] = {
    "direct", "indirect", "launch_surface", "own_surface", "mu_zero", "mu_finite", "mu_inf", "soft_erp_on", "soft_erp_off", "soft_cfm_on",
    "soft_cfm_off", "bounce_off", "bounce_taken", "bounce_below_vel", "layer_zero", "layer_above_depth", "maxcorr_inf", "maxcorr_binds",
    "negative_depth" };

template <class T> static bool same_bits(T a, T b) { return memcmp(&a, &b, sizeof(T)) == 0; }

template <class T> static int run(const char *name, int n_cases, uint64_t seed)
{
    constexpr int NCON = 4;             // contacts in the tables; one of them is the case's
    Rng rng = { seed };
    long cov[COV_COUNT] = {};
    int bad = 0;
    long rows_compared = 0;
    std::vector<T> S((size_t)C_COUNT * SLAB_TILE, T(0));
    std::vector<int> local(SLAB_TILE, 0);
    const T inf = Limits<T>::inf();
    for (int n = 0; n < n_cases; n++) {
        const int s = rng.pick(SLAB_TILE), ci = rng.pick(NCON);
        const bool ind = rng.pick(2) == 1, own = rng.pick(2) == 1;
        const V3<T> x1 = { (T)rng.uni(-2, 2), (T)rng.uni(0.2, 1.5), (T)rng.uni(-2, 2) };
        // the approach speed along the normal lies on either side of bounce_vel (0.3): -0.05 .. -0.8 along y, the normal near y
        const V3<T> v1 = { (T)rng.uni(-1, 1), (T)rng.uni(-0.8, -0.05), (T)rng.uni(-1, 1) };
        const V3<T> w1 = { (T)rng.uni(-0.3, 0.3), (T)rng.uni(-0.3, 0.3), (T)rng.uni(-0.3, 0.3) };
        const T xs[3] = { x1.x, x1.y, x1.z }, vs[3] = { v1.x, v1.y, v1.z }, ws[3] = { w1.x, w1.y, w1.z };
        for (int k = 0; k < 3; k++) {
            S[(size_t)slab_ix(C_POS + k, s)] = xs[k]; S[(size_t)slab_ix(C_LVEL + k, s)] = vs[k]; S[(size_t)slab_ix(C_AVEL + k, s)] = ws[k];
        }
        // the tables: the direct ones by contact, the indirect ones where csrc points (a permutation, so that a mixed-up index shows)
        T cpos[3 * NCON], cnormal[3 * NCON], cdepth[NCON], gpos[3 * NCON], gnormal[3 * NCON], gdepth[NCON];
        T cmu[NCON], cbounce[NCON], cbv[NCON], cserp[NCON], cscfm[NCON];
        int csrc[NCON], cb1[NCON], cb2[NCON], cmode[NCON];
        const int rot = 1 + rng.pick(NCON - 1);
        const T mus[3] = { T(0), (T)rng.uni(0.1, 1.5), inf };
        for (int c = 0; c < NCON; c++) {
            csrc[c] = (c + rot) % NCON; cb1[c] = s; cb2[c] = -1;
            double nx = rng.uni(-0.3, 0.3), nz = rng.uni(-0.3, 0.3), nl = sqrt(nx * nx + 1.0 + nz * nz);
            const T nrm[3] = { (T)(nx / nl), (T)(1.0 / nl), (T)(nz / nl) };
            const T pos[3] = { (T)(x1.x + rng.uni(-0.5, 0.5)), (T)(x1.y - rng.uni(0.1, 0.6)), (T)(x1.z + rng.uni(-0.5, 0.5)) };
            const T depth = (T)rng.uni(-0.005, 0.03);
            T *tp = ind ? gpos + 3 * csrc[c] : cpos + 3 * c, *tn = ind ? gnormal + 3 * csrc[c] : cnormal + 3 * c;
            for (int k = 0; k < 3; k++) { tp[k] = pos[k]; tn[k] = nrm[k]; }
            // (the table that is not in use holds other numbers: reading it shows)
            T *up = ind ? cpos + 3 * c : gpos + 3 * c, *un = ind ? cnormal + 3 * c : gnormal + 3 * c;
            for (int k = 0; k < 3; k++) { up[k] = (T)rng.uni(-9, 9); un[k] = (T)rng.uni(-1, 1); }
            if (ind) { gdepth[csrc[c]] = depth; cdepth[c] = (T)rng.uni(1, 2); }
            else { cdepth[c] = depth; gdepth[c] = (T)rng.uni(1, 2); }
            cmode[c] = (rng.pick(2) ? SURF_SOFT_ERP : 0) | (rng.pick(2) ? SURF_SOFT_CFM : 0) | (rng.pick(2) ? SURF_BOUNCE : 0);
            cmu[c] = mus[rng.pick(3)];
            cbounce[c] = (T)rng.uni(0.1, 0.9); cbv[c] = (T)0.3; cserp[c] = (T)rng.uni(0.05, 0.9); cscfm[c] = (T)rng.uni(1e-6, 1e-2);
        }
        StepParams<T> P = {};
        P.h = (T)(1.0 / 60.0); P.erp = (T)0.2; P.cfm = (T)1e-5; P.sor_w = (T)1.3;
        P.mu = mus[rng.pick(3)]; P.surf_mode = cmode[rng.pick(NCON)]; P.bounce = (T)0.5; P.bounce_vel = (T)0.3;
        IslandSet<T> I = {};
        I.n_islands = 1;
        I.cpos = cpos; I.cnormal = cnormal; I.cdepth = cdepth;
        if (ind) { I.csrc = csrc; I.gpos = gpos; I.gnormal = gnormal; I.gdepth = gdepth; }
        I.cb1 = cb1; I.cb2 = cb2; I.cmode = cmode; I.local = local.data();
        if (own) { I.cmu = cmu; I.cbounce = cbounce; I.cbounce_vel = cbv; I.csoft_erp = cserp; I.csoft_cfm = cscfm; }
        I.surface_layer = rng.pick(2) ? (T)0.01 : T(0);
        I.max_corr_vel = rng.pick(2) ? (T)0.05 : inf;
        const T hinv = T(1) / P.h;

        // the general path's rows
        T rows[3 * RW_COUNT];
        int jb[6];
        for (int k = 0; k < 3 * RW_COUNT; k++) rows[k] = (T)-77;
        contact_rows<T>(S.data(), (int64_t)SLAB_TILE, I, P, rows, jb, ci, 0, hinv);

        // the one-body forms'
        size_t gi;
        V3<T> c1, dir[3];
        int mode, rpc;
        T lo_f, hi_f;
        single_contact(I, P, ci, x1, gi, c1, mode, rpc, dir, lo_f, hi_f);
        const T mu = own ? cmu[ci] : P.mu;
        bool ok = rpc == (mu > 0 ? 3 : 1);
        for (int d = 0; d < rpc && ok; d++) {
            T J[6], cval, cfm;
            single_contact_row(I, P, ci, gi, mode, d == 0, c1, dir[d], v1, w1, hinv, J, cval, cfm);
            const T *row = rows + (size_t)d * RW_COUNT;
            for (int j = 0; j < 6; j++) ok = ok && same_bits(J[j], row[RW_J + j]);
            ok = ok && same_bits(cval, row[RW_RHS]) && same_bits(cfm, row[RW_AD]);
            ok = ok && same_bits(d == 0 ? T(0) : lo_f, row[RW_LO]) && same_bits(d == 0 ? inf : hi_f, row[RW_HI]);
            rows_compared++;
        }
        if (!ok && bad++ < 5)
            fprintf(stderr, "%s case %d: rows differ (indirect %d, own surface %d, mode 0x%x, mu %g, rpc %d)\n", name, n, (int)ind, (int)own, mode, (double)mu, rpc);

        // what this case covered, judged from its inputs (in double: classes, not bits)
        const double depth = (double)(ind ? gdepth[gi] : cdepth[ci]), layer = (double)I.surface_layer;
        const double erp = (mode & SURF_SOFT_ERP) ? (own ? (double)cserp[ci] : 0.0) : (double)P.erp;
        const double left = depth - layer > 0 ? depth - layer : 0.0, c_plain = (double)hinv * erp * left;
        cov[ind ? COV_INDIRECT : COV_DIRECT]++; cov[own ? COV_OWN_SURFACE : COV_LAUNCH_SURFACE]++;
        cov[mu > 0 ? (mu < inf ? COV_MU_FINITE : COV_MU_INF) : COV_MU_ZERO]++;
        cov[(mode & SURF_SOFT_ERP) ? COV_SOFT_ERP_ON : COV_SOFT_ERP_OFF]++; cov[(mode & SURF_SOFT_CFM) ? COV_SOFT_CFM_ON : COV_SOFT_CFM_OFF]++;
        if (mode & SURF_BOUNCE) {
            const double out = (double)rows[RW_J + 0] * v1.x + (double)rows[RW_J + 1] * v1.y + (double)rows[RW_J + 2] * v1.z +
                               (double)rows[RW_J + 3] * w1.x + (double)rows[RW_J + 4] * w1.y + (double)rows[RW_J + 5] * w1.z;
            cov[-out > 0.3 + 1e-3 ? COV_BOUNCE_TAKEN : COV_BOUNCE_BELOW_VEL]++;
        } else cov[COV_BOUNCE_OFF]++;
        if (layer == 0) cov[COV_LAYER_ZERO]++;
        else if (depth > 0 && layer > depth) cov[COV_LAYER_ABOVE_DEPTH]++;
        if (I.max_corr_vel == inf) cov[COV_MAXCORR_INF]++;
        else if (c_plain > (double)I.max_corr_vel) cov[COV_MAXCORR_BINDS]++;
        if (depth < 0) cov[COV_NEGATIVE_DEPTH]++;
    }
    printf("%s: %d contacts, %ld rows compared, %d contacts with a difference\n", name, n_cases, rows_compared, bad);
    for (int k = 0; k < COV_COUNT; k++) {
        printf("%s coverage %s %ld\n", name, cov_name[k], cov[k]);
        if (cov[k] == 0) { fprintf(stderr, "%s: the population never met %s\n", name, cov_name[k]); bad++; }
    }
    return bad;
}

int main(int argc, char **argv)
{
    const int n = argc > 1 ? atoi(argv[1]) : 4096;
    if (n < 1) { fprintf(stderr, "usage: single_contact_harness [contacts per precision]\n"); return 2; }
    const int bad = run<float>("float", n, 0x9E3779B97F4A7C15ull) + run<double>("double", n, 0xD1B54A32D192ED03ull);
    return bad ? 1 : 0;
}
