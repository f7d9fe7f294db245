// Stand-alone host program for tests/test_launch_consts.py: the rule of csrc/dmx_launch_consts.hpp, the constants it computes, and
// the general tick of csrc/dmx_step_fused.hpp fed those constants (free_body_step_with over TickGiven) against the same tick dividing
// per body (free_body_step, over TickDivides).  Built with hipcc for the host and the product's flags; no GPU, no HIP call.
//   launch_consts_harness [bodies per precision, default 65536]
// Prints one line per check and exits 0 only if every one holds.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "dmx_math.hpp"
#include "dmx_step_fused.hpp"
#include "dmx_torque_free.hpp"
#include "dmx_launch_consts.hpp"

using namespace dmx;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

template <class T> struct Name;
template <> struct Name<float>  { static const char *s() { return "f32"; } };
template <> struct Name<double> { static const char *s() { return "f64"; } };
template <class T> static uint64_t bits(T v) { uint64_t u = 0; memcpy(&u, &v, sizeof(T)); return u; }
template <class T> static T from_bits(uint64_t u) { T v; memcpy(&v, &u, sizeof(T)); return v; }
template <class T> static T denormal() { return from_bits<T>(12345); }               // a denormal of T whose reciprocal is infinite
template <class T> static T tiny_normal() { return from_bits<T>(sizeof(T) == 4 ? 0x00800000ull : 0x0010000000000000ull); }

struct Rng {            // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
    double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }         // [0, 1)
    double sym(double a) { return (2.0 * uni() - 1.0) * a; }
};

template <class T> static int rule_on(T m, T i0, T i1, T i2, T h)
{
    const T Ib[3] = { i0, i1, i2 };
    return launch_consts<T>(m, Ib, h).on;
}

template <class T> static void truth_table()
{
    const T h = T(1) / T(60), inf = Limits<T>::inf(), nan = Limits<T>::nan();
    const int before = failures;
    CHECK(rule_on<T>(1, 1, 1, 1, h) == 1, "%s: m = 1, I = identity must be on", Name<T>::s());
    CHECK(rule_on<T>(T(2.5), T(0.3), T(1.7), T(0.9), h) == 1, "%s: m = 2.5, I = (0.3, 1.7, 0.9) must be on", Name<T>::s());
    CHECK(rule_on<T>(T(-2.5), T(0.3), T(-1.7), T(0.9), h) == 1, "%s: negative finite constants have finite reciprocals: on", Name<T>::s());
    CHECK(rule_on<T>(tiny_normal<T>(), 1, 1, 1, h) == 1, "%s: the smallest normal number has a finite reciprocal: on", Name<T>::s());
    const T bad[] = { T(0), -T(0), denormal<T>(), -denormal<T>(), inf, -inf, nan };
    for (T b : bad) {
        CHECK(rule_on<T>(b, 1, 1, 1, h) == 0, "%s: m = %g must be off", Name<T>::s(), (double)b);
        for (int k = 0; k < 3; k++) {
            T I[3] = { T(0.3), T(1.7), T(0.9) };
            I[k] = b;
            CHECK(rule_on<T>(T(2.5), I[0], I[1], I[2], h) == 0, "%s: inertia %g in component %d must be off", Name<T>::s(), (double)b, k);
        }
    }
    for (T hb : { T(0), -T(0), inf, -inf, nan, denormal<T>() })
        CHECK(rule_on<T>(1, 1, 1, 1, hb) == 0, "%s: h = %g must be off", Name<T>::s(), (double)hb);
    printf("%s truth table: %s\n", Name<T>::s(), failures == before ? "ok" : "FAILED");
}

template <class T> static void constants()
{
    const int before = failures;
    Rng r{ 99 };
    const T special[] = { T(1), T(0), -T(0), T(0.5), T(3), denormal<T>(), tiny_normal<T>(), Limits<T>::inf(), Limits<T>::nan(), (T)1e19, (T)3e38, T(-2.5) };
    const int ns = (int)(sizeof(special) / sizeof(special[0]));
    int on = 0;
    for (int it = 0; it < 20000; it++) {
        const T m = it % 3 == 0 ? special[r.next() % ns] : (T)(0.01 + 10.0 * r.uni());
        const T h = it % 5 == 0 ? special[r.next() % ns] : (T)(1e-4 + 0.1 * r.uni());
        T Ib[3];
        for (int k = 0; k < 3; k++) Ib[k] = it % 7 == 0 ? special[r.next() % ns] : (T)(0.05 + 5.0 * r.uni());
        if (it % 4 == 1) Ib[1] = Ib[2] = Ib[0];
        const LaunchConsts<T> lc = launch_consts<T>(m, Ib, h);
        on += lc.on;
        // as TickDivides (dmx_step_fused.hpp) and add_gyro_torque (dmx_math.hpp) spell them
        const TickDivides<T> D = { m, { Ib[0], Ib[1], Ib[2] }, h };
        const V3<T> invIb = D.invIb();
        CHECK(bits(lc.inv_Ib[0]) == bits(invIb.x) && bits(lc.inv_Ib[1]) == bits(invIb.y) && bits(lc.inv_Ib[2]) == bits(invIb.z),
              "%s: 1 / Ib of (%g, %g, %g)", Name<T>::s(), (double)Ib[0], (double)Ib[1], (double)Ib[2]);
        CHECK(bits(lc.inv_Ib[0]) == bits(T(1) / Ib[0]), "%s: 1 / Ib.x of %g", Name<T>::s(), (double)Ib[0]);
        CHECK(bits(lc.inv_m) == bits(T(1) / m), "%s: 1 / m of %g", Name<T>::s(), (double)m);
        CHECK(bits(lc.inv_h) == bits(D.hinv_of()()) && bits(lc.inv_h) == bits(T(1) / h), "%s: 1 / h of %g", Name<T>::s(), (double)h);
        CHECK((lc.iso != 0) == D.iso(), "%s: isotropy of (%g, %g, %g)", Name<T>::s(), (double)Ib[0], (double)Ib[1], (double)Ib[2]);
        // hm travels in TorqueFree: the product of the launch's h and this 1 / m
        const T g[3] = { 0, T(-9.81), 0 };
        CHECK(bits(torque_free_plan<T>(true, true, false, 0, m, Ib, h, g).hm) == bits(h * lc.inv_m) && bits(h * lc.inv_m) == bits(D.hm()),
              "%s: hm of h = %g, m = %g", Name<T>::s(), (double)h, (double)m);
        // the rule, restated: finite, not zero, reciprocal finite
        bool want = true;
        for (T v : { m, Ib[0], Ib[1], Ib[2], h }) {
            const T rec = T(1) / v;
            want = want && v == v && v != Limits<T>::inf() && v != -Limits<T>::inf() && v != T(0) && rec != Limits<T>::inf() && rec != -Limits<T>::inf();
        }
        CHECK((lc.on != 0) == want, "%s: the rule on m = %g, Ib = (%g, %g, %g), h = %g", Name<T>::s(), (double)m, (double)Ib[0], (double)Ib[1], (double)Ib[2], (double)h);
    }
    CHECK(on > 5000 && on < 19000, "%s: %d of 20000 launches admitted: the cases do not exercise both answers", Name<T>::s(), on);
    printf("%s constants: %s\n", Name<T>::s(), failures == before ? "ok" : "FAILED");
}

template <class T> static void ticks(int64_t n)
{
    const int before = failures;
    Rng r{ sizeof(T) == 4 ? 515u : 1030u };
    const T inf = Limits<T>::inf();
    const T special[] = { T(0), -T(0), denormal<T>(), -denormal<T>(), inf, -inf, Limits<T>::nan(), (T)1e19, (T)-1e19, (T)3e38, (T)-3e38 };
    const int ns = (int)(sizeof(special) / sizeof(special[0]));
    struct Launch { T m, I[3], h, g[3]; };
    const Launch launches[] = {
        { 1, { 1, 1, 1 }, T(1) / T(60), { 0, T(-9.81), 0 } },
        { T(2.5), { T(0.3), T(1.7), T(0.9) }, T(1) / T(60), { 0, T(-9.81), 0 } },
        { T(40), { T(1e6), T(2e6), T(1e-6) }, T(0.1), { T(0.3), T(-9.81), T(-1.1) } },
        { T(1e-3), { T(0.4), T(0.4), T(3.1) }, T(1) / T(240), { 0, 0, T(-1.62) } },
        { T(7), { T(2), T(2), T(2) }, T(0.01), { 0, -0.0f, 0 } },
    };
    const int nl = (int)(sizeof(launches) / sizeof(launches[0]));
    int64_t differ = 0, with_acc = 0, gyro_ran = 0, nan_pairs = 0;
    for (int64_t i = 0; i < n; i++) {
        const Launch &L = launches[i % nl];
        const int gyro = (int)((i / nl) % 3);
        const V3<T> Ib = { L.I[0], L.I[1], L.I[2] }, g = { L.g[0], L.g[1], L.g[2] };
        const LaunchConsts<T> lc = launch_consts<T>(L.m, L.I, L.h);
        const TorqueFree<T> tf = torque_free_plan<T>(true, true, false, gyro, L.m, L.I, L.h, L.g);
        if (i < 3 * nl) CHECK(lc.on == 1, "%s: launch %d must be admitted by the rule", Name<T>::s(), (int)(i % nl));
        T c[13];
        for (int k = 0; k < 3; k++) c[k] = (T)r.sym(100.0);
        double qn = 0, qq[4];
        for (int k = 0; k < 4; k++) { qq[k] = r.sym(1.0); qn += qq[k] * qq[k]; }
        const double scale = (i & 15) == 5 ? 1.0 + 3.0 * r.uni() : 1.0;          // some not normalised, beyond the short tick's guard too
        for (int k = 0; k < 4; k++) c[3 + k] = (T)(qq[k] / (qn > 0 ? __builtin_sqrt(qn) : 1.0) * scale);
        for (int k = 0; k < 3; k++) c[7 + k] = (T)r.sym(10.0);
        for (int k = 0; k < 3; k++) c[10 + k] = (T)r.sym(30.0);
        const bool planted = (i & 7) == 3;
        if (planted) {                                                           // an eighth of them: special values planted
            const int np = 1 + (int)(r.next() % 3);
            for (int p = 0; p < np; p++) c[r.next() % 13] = special[r.next() % ns];
        }
        const bool acc = (i & 3) == 2;                                           // a quarter with force and torque accumulators set
        V3<T> facc = { T(0), T(0), T(0) }, tacc = { T(0), T(0), T(0) };
        if (acc) { facc = { (T)r.sym(5.0), (T)r.sym(5.0), (T)r.sym(5.0) }; tacc = { (T)r.sym(2.0), (T)r.sym(2.0), (T)r.sym(2.0) }; with_acc++; }
        gyro_ran += gyro != 0 && !isotropic(Ib);
        V3<T> x = { c[0], c[1], c[2] }, v = { c[7], c[8], c[9] }, w = { c[10], c[11], c[12] };
        Q4<T> q = { c[3], c[4], c[5], c[6] };
        V3<T> x2 = x, v2 = v, w2 = w;
        Q4<T> q2 = q;
        // the tick that divides, as every kernel without the constants runs it
        free_body_step(x, q, v, w, L.m, Ib, facc, tacc, g, L.h, gyro);
        // the tick fed the host's constants, as integrate_free's instantiations with OPT_UNI run it: with accumulators, and without
        const V3<T> inv = { lc.inv_Ib[0], lc.inv_Ib[1], lc.inv_Ib[2] }, mg = { tf.mg[0], tf.mg[1], tf.mg[2] };
        if (acc) free_body_step_with(x2, q2, v2, w2, Ib, facc, tacc, g, L.h, gyro, TickGiven<T, true>{ inv, lc.iso != 0, lc.inv_h, tf.hm, L.m, mg });
        else free_body_step_with(x2, q2, v2, w2, Ib, facc, tacc, g, L.h, gyro, TickGiven<T, false>{ inv, lc.iso != 0, lc.inv_h, tf.hm, L.m, mg });
        const T a[13] = { x.x, x.y, x.z, q.w, q.x, q.y, q.z, v.x, v.y, v.z, w.x, w.y, w.z };
        const T b[13] = { x2.x, x2.y, x2.z, q2.w, q2.x, q2.y, q2.z, v2.x, v2.y, v2.z, w2.x, w2.y, w2.z };
        // bit for bit; where a planted inf or NaN has made a component NaN in both, its sign and payload are the host processor's choice
        // between two NaN operands in whatever order the compiler left them, not the tick's: both must be NaN, and only there
        bool same = true;
        for (int k = 0; k < 13; k++) {
            const bool both_nan = a[k] != a[k] && b[k] != b[k];
            if (both_nan && !planted) same = false;
            nan_pairs += both_nan;
            same = same && (bits(a[k]) == bits(b[k]) || both_nan);
        }
        if (!same && differ++ < 5)
            for (int k = 0; k < 13; k++)
                if (bits(a[k]) != bits(b[k]))
                    printf("  %s body %lld (launch %d, gyro %d) component %d: dividing %a given %a (loaded %a)\n", Name<T>::s(), (long long)i,
                           (int)(i % nl), gyro, k, (double)a[k], (double)b[k], (double)c[k]);
    }
    CHECK(differ == 0, "%s: %lld of %lld bodies differ between the dividing tick and the tick given the constants", Name<T>::s(), (long long)differ, (long long)n);
    CHECK(with_acc * 5 > n && gyro_ran * 4 > n, "%s: %lld bodies with accumulators, %lld with a gyroscopic torque: too few", Name<T>::s(),
          (long long)with_acc, (long long)gyro_ran);
    printf("%s ticks: %lld bodies, %lld with accumulators, %lld with a gyroscopic torque, %lld components NaN in both (planted values only), %lld differ: %s\n",
           Name<T>::s(), (long long)n, (long long)with_acc, (long long)gyro_ran, (long long)nan_pairs, (long long)differ, failures == before ? "ok" : "FAILED");
}

int main(int argc, char **argv)
{
    const int64_t n = argc > 1 ? atoll(argv[1]) : 65536;
    truth_table<float>(); truth_table<double>();
    constants<float>(); constants<double>();
    ticks<float>(n); ticks<double>(n);
    printf(failures == 0 ? "launch_consts_harness: all checks hold\n" : "launch_consts_harness: %d checks FAILED\n", failures);
    return failures == 0 ? 0 : 1;
}
