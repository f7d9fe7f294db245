// autodisable_harness.cpp -- csrc/dmx_autodisable.hpp's idle_update on the host, in the precision chosen at compile time
// (-DROWS_SINGLE: float), as an evaluator for tests/test_autodisable_harness.py: the function the end-of-tick pass and the
// single-launch tick call per stepped slot, fed from a slab of a few tiles.
//
//   autodisable_harness <cases.bin> <out.bin>
// cases.bin  five doubles (lin_threshold, ang_threshold, idle_steps, idle_time, h), then records of 9 doubles: lvel3 avel3 flags
//            steps_left time_left, one per slot
// out.bin    records of 10 doubles: lvel3 avel3 flags steps_left time_left and the byte idle_update returned
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "dmx_autodisable.hpp"

#ifdef ROWS_SINGLE
typedef float real;
#else
typedef double real;
#endif
using namespace dmx;

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: autodisable_harness <cases.bin> <out.bin>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    double head[5];
    if (fread(head, sizeof(double), 5, f) != 5) { fprintf(stderr, "no header in %s\n", argv[1]); return 2; }
    std::vector<double> in;
    double rec[9];
    while (fread(rec, sizeof(double), 9, f) == 9) in.insert(in.end(), rec, rec + 9);
    fclose(f);
    const int n = (int)(in.size() / 9);
    const int stride = (n + SLAB_TILE - 1) / SLAB_TILE * SLAB_TILE;
    std::vector<real> S((size_t)C_COUNT * stride, real(0));
    std::vector<uint8_t> flags((size_t)stride, 0);
    std::vector<int32_t> steps((size_t)stride, 0);
    std::vector<double> time((size_t)stride, 0.0);
    for (int s = 0; s < n; s++) {
        const double *r = in.data() + (size_t)9 * s;
        for (int c = 0; c < 6; c++) S[(size_t)slab_ix(C_LVEL + c, s)] = (real)r[c];
        flags[(size_t)s] = (uint8_t)r[6]; steps[(size_t)s] = (int32_t)r[7]; time[(size_t)s] = r[8];
    }
    const IdleParams<real> A = make_idle_params<real>(head[0], head[1], (int)head[2], head[3], head[4]);
    FILE *o = fopen(argv[2], "wb");
    if (!o) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    for (int s = 0; s < n; s++) {
        const uint8_t got = idle_update<real>(S.data(), flags.data(), steps.data(), time.data(), A, s);
        double out[10];
        for (int c = 0; c < 6; c++) out[c] = S[(size_t)slab_ix(C_LVEL + c, s)];
        out[6] = flags[(size_t)s]; out[7] = steps[(size_t)s]; out[8] = time[(size_t)s]; out[9] = got;
        fwrite(out, sizeof(double), 10, o);
    }
    fclose(o);
    return 0;
}
