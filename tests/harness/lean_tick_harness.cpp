// Stand-alone host program for tests/test_lean_tick.py: the straight-line tick of csrc/dmx_lean_tick.hpp (lean_tick: what
// integrate_free_lean runs for a tile whose lateral axes are fixed) against torque_free_step fed the same body with
// v.x = v.z = x.x = x.z = 0 and mg.x = mg.z = +0, and against free_body_step (csrc/dmx_step_fused.hpp: the general tick, dividing
// per body, gyro mode 0, no accumulators) on every body torque_free_admits admits.  Built with hipcc for the host and the product's flags; no GPU, no HIP call.
//   lean_tick_harness [bodies per precision, default 1048576]
// Prints one line per check and exits 0 only if every one holds.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "dmx_math.hpp"
#include "dmx_step_fused.hpp"
#include "dmx_torque_free.hpp"
#include "dmx_lean_tick.hpp"

using namespace dmx;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

template <class T> struct Name;
template <> struct Name<float>  { static const char *s() { return "f32"; } };
template <> struct Name<double> { static const char *s() { return "f64"; } };
template <class T> static uint64_t bits(T v) { uint64_t u = 0; memcpy(&u, &v, sizeof(T)); return u; }
template <class T> static T from_bits(uint64_t u) { T v; memcpy(&v, &u, sizeof(T)); return v; }
template <class T> static T denormal() { return from_bits<T>(12345); }
template <class T> static T snan() { return from_bits<T>(sizeof(T) == 4 ? 0x7fa00001ull : 0x7ff4000000000001ull); }

struct Rng {            // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
    double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
    double sym(double a) { return (2.0 * uni() - 1.0) * a; }
};

template <class T> static void ticks(int64_t n)
{
    const int before = failures;
    Rng r{ sizeof(T) == 4 ? 515u : 1030u };
    const T inf = Limits<T>::inf();
    const T special[] = { T(0), -T(0), denormal<T>(), -denormal<T>(), inf, -inf, Limits<T>::nan(), snan<T>(), (T)1e19, (T)-1e19, (T)3e38, (T)-3e38 };
    const int ns = (int)(sizeof(special) / sizeof(special[0]));
    // launches the rule admits, gravity along y alone (what keeps a tile's lateral axes fixed)
    struct Launch { T m, I[3], h, gy; };
    const Launch launches[] = {
        { 1, { 1, 1, 1 }, T(1) / T(60), T(-9.81) },
        { T(2.5), { T(0.4), T(1.7), T(3.1) }, T(0.01), T(-9.81) },
        { T(1e-3), { T(1), T(1), T(1) }, T(1) / T(240), T(-1.62) },
        { T(40), { T(1e6), T(2e6), T(1e-6) }, T(0.1), T(3.7) },
    };
    int64_t admitted = 0, differ_short = 0, differ_general = 0, planted = 0;
    for (int64_t i = 0; i < n; i++) {
        const Launch &L = launches[i & 3];
        const T g[3] = { T(0), L.gy, T(0) };
        const TorqueFree<T> tf = torque_free_plan<T>(true, true, false, 0, L.m, L.I, L.h, g);
        if (i < 4) {
            CHECK(tf.on == 1, "%s: launch %d must be admitted by the rule", Name<T>::s(), (int)i);
            CHECK(bits(tf.mg[0]) == bits(T(0)) && bits(tf.mg[2]) == bits(T(0)), "%s: launch %d: mg.x and mg.z must be +0", Name<T>::s(), (int)i);
        }
        // the nine components a lean tile loads: pos.y, quat, lvel.y, avel
        T c[9];
        c[0] = (T)r.sym(100.0);
        double qn = 0, qq[4];
        for (int k = 0; k < 4; k++) { qq[k] = r.sym(1.0); qn += qq[k] * qq[k]; }
        const double scale = (i & 15) == 5 ? 1.0 + r.uni() : 1.0;          // some not normalised, up to |q.k| < 2
        for (int k = 0; k < 4; k++) c[1 + k] = (T)(qq[k] / (qn > 0 ? __builtin_sqrt(qn) : 1.0) * scale);
        c[5] = (T)r.sym(10.0);
        for (int k = 0; k < 3; k++) c[6 + k] = (T)r.sym(30.0);
        if ((i & 3) == 3) {                                                // a quarter of them: special values planted in q, w, v.y, x.y
            const int np = 1 + (int)(r.next() % 3);
            for (int p = 0; p < np; p++) c[r.next() % 9] = special[r.next() % ns];
            planted++;
        }
        // the straight-line tick
        T xy = c[0], vy = c[5];
        Q4<T> q = { c[1], c[2], c[3], c[4] };
        V3<T> w = { c[6], c[7], c[8] };
        lean_tick(xy, q, vy, w, tf.hm, tf.mg[1], L.h);
        // torque_free_step on the same body with the lateral axes at zero and mg.x = mg.z = +0
        V3<T> x2 = { T(0), c[0], T(0) }, v2 = { T(0), c[5], T(0) }, w2 = { c[6], c[7], c[8] };
        Q4<T> q2 = { c[1], c[2], c[3], c[4] };
        torque_free_step(x2, q2, v2, w2, tf.hm, V3<T>{ T(0), tf.mg[1], T(0) }, L.h);
        const T a[9] = { xy, q.w, q.x, q.y, q.z, vy, w.x, w.y, w.z };
        const T b[9] = { x2.y, q2.w, q2.x, q2.y, q2.z, v2.y, w2.x, w2.y, w2.z };
        bool same = true;
        for (int k = 0; k < 9; k++) same = same && bits(a[k]) == bits(b[k]);
        if (!same && differ_short++ < 5)
            for (int k = 0; k < 9; k++)
                if (bits(a[k]) != bits(b[k]))
                    printf("  %s body %lld component %d: lean %a torque_free_step %a (loaded %a)\n", Name<T>::s(), (long long)i, k, (double)a[k], (double)b[k], (double)c[k]);
        // ... and the general tick, on every body the guard admits
        const Q4<T> q0 = { c[1], c[2], c[3], c[4] };
        if (torque_free_admits(q0)) {
            admitted++;
            V3<T> x3 = { T(0), c[0], T(0) }, v3 = { T(0), c[5], T(0) }, w3 = { c[6], c[7], c[8] };
            Q4<T> q3 = q0;
            const V3<T> zero = { T(0), T(0), T(0) };
            free_body_step(x3, q3, v3, w3, L.m, V3<T>{ L.I[0], L.I[1], L.I[2] }, zero, zero, V3<T>{ g[0], g[1], g[2] }, L.h, 0);
            const T d[9] = { x3.y, q3.w, q3.x, q3.y, q3.z, v3.y, w3.x, w3.y, w3.z };
            bool same3 = true;
            for (int k = 0; k < 9; k++) same3 = same3 && bits(a[k]) == bits(d[k]);
            if (!same3 && differ_general++ < 5)
                for (int k = 0; k < 9; k++)
                    if (bits(a[k]) != bits(d[k]))
                        printf("  %s body %lld component %d: lean %a general %a (loaded %a)\n", Name<T>::s(), (long long)i, k, (double)a[k], (double)d[k], (double)c[k]);
        }
    }
    CHECK(differ_short == 0, "%s: %lld of %lld bodies differ from torque_free_step", Name<T>::s(), (long long)differ_short, (long long)n);
    CHECK(differ_general == 0, "%s: %lld of %lld admitted bodies differ from the general tick", Name<T>::s(), (long long)differ_general, (long long)admitted);
    CHECK(admitted * 10 > n * 8 && admitted < n, "%s: %lld of %lld bodies admitted", Name<T>::s(), (long long)admitted, (long long)n);
    CHECK(planted * 4 == n - (n & 3), "%s: %lld of %lld bodies carry planted values", Name<T>::s(), (long long)planted, (long long)n);
    printf("%s ticks: %lld bodies, %lld with planted values, %lld differ from torque_free_step, %lld admitted of which %lld differ from the general tick: %s\n",
           Name<T>::s(), (long long)n, (long long)planted, (long long)differ_short, (long long)admitted, (long long)differ_general, failures == before ? "ok" : "FAILED");
}

int main(int argc, char **argv)
{
    const int64_t n = argc > 1 ? atoll(argv[1]) : 1048576;
    ticks<float>(n); ticks<double>(n);
    printf(failures == 0 ? "lean_tick_harness: all checks hold\n" : "lean_tick_harness: %d checks FAILED\n", failures);
    return failures == 0 ? 0 : 1;
}
