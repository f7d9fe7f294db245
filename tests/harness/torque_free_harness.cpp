// Stand-alone host program for tests/test_torque_free.py: the rule of csrc/dmx_torque_free.hpp and the short tick of
// csrc/dmx_math.hpp (torque_free_step behind torque_free_admits) against the general tick, restated here from quat_to_R,
// rotate_diag, mulv and integrate_quat.  Built with hipcc for the host and the product's flags; no GPU, no HIP call.
//   torque_free_harness [bodies per precision, default 1048576]
// Prints one line per check and exits 0 only if every one holds.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "dmx_math.hpp"
#include "dmx_torque_free.hpp"

using namespace dmx;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

template <class T> struct Name;
template <> struct Name<float>  { static const char *s() { return "f32"; } };
template <> struct Name<double> { static const char *s() { return "f64"; } };
template <class T> static uint64_t bits(T v) { uint64_t u = 0; memcpy(&u, &v, sizeof(T)); return u; }
template <class T> static T from_bits(uint64_t u) { T v; memcpy(&v, &u, sizeof(T)); return v; }
template <class T> static T denormal() { return from_bits<T>(12345); }               // a denormal of T
template <class T> static T snan() { return from_bits<T>(sizeof(T) == 4 ? 0x7fa00001ull : 0x7ff4000000000001ull); }

struct Rng {            // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
    double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }         // [0, 1)
    double sym(double a) { return (2.0 * uni() - 1.0) * a; }
};

template <class T> static int plan_on(bool enabled, bool uni, bool ext, int gyro, T m, T i0, T i1, T i2, T h)
{
    const T Ib[3] = { i0, i1, i2 }, g[3] = { T(0), T(-9.81), T(0) };
    return torque_free_plan<T>(enabled, uni, ext, gyro, m, Ib, h, g).on;
}

template <class T> static void truth_table()
{
    const T h = T(1) / T(60), inf = Limits<T>::inf(), nan = Limits<T>::nan();
    const int before = failures;
    CHECK(plan_on<T>(true, true, false, 2, 1, 1, 1, 1, h) == 1, "%s: m = 1, I = identity must be on", Name<T>::s());
    CHECK(plan_on<T>(true, true, false, 1, 1, 1, 1, 1, h) == 1, "%s: isotropic with gyro 1 must be on", Name<T>::s());
    CHECK(plan_on<T>(true, true, false, 0, 1, 1, 1, 1, h) == 1, "%s: isotropic with gyro 0 must be on", Name<T>::s());
    CHECK(plan_on<T>(true, true, false, 1, 1, 1, 2, 3, h) == 0, "%s: anisotropic with gyro 1 must be off", Name<T>::s());
    CHECK(plan_on<T>(true, true, false, 2, 1, 1, 2, 3, h) == 0, "%s: anisotropic with gyro 2 must be off", Name<T>::s());
    CHECK(plan_on<T>(true, true, false, 2, 1, 2, 2, 3, h) == 0, "%s: anisotropic in one component with gyro 2 must be off", Name<T>::s());
    CHECK(plan_on<T>(true, true, false, 0, 1, 1, 2, 3, h) == 1, "%s: anisotropic with gyro 0 must be on", Name<T>::s());
    CHECK(plan_on<T>(true, true, true, 2, 1, 1, 1, 1, h) == 0, "%s: accumulators set must be off", Name<T>::s());
    CHECK(plan_on<T>(true, false, false, 2, 1, 1, 1, 1, h) == 0, "%s: non-uniform constants must be off", Name<T>::s());
    CHECK(plan_on<T>(false, true, false, 2, 1, 1, 1, 1, h) == 0, "%s: the switch off must be off", Name<T>::s());
    const T bad[] = { T(0), -T(0), T(-1), (T)1e-40f, denormal<T>(), nan, -inf };
    for (T b : bad)
        for (int k = 0; k < 3; k++) {
            T I[3] = { 1, 1, 1 };
            I[k] = b;
            // (1e-40, a denormal of f32, is a normal number of f64 with a finite inverse far below the bound: the rule says on there)
            const int want = (sizeof(T) == 8 && b == (T)1e-40f) ? 1 : 0;
            CHECK(plan_on<T>(true, true, false, 0, 1, I[0], I[1], I[2], h) == want, "%s: inertia %g in component %d must be %s",
                  Name<T>::s(), (double)b, k, want ? "on" : "off");
        }
    // the bound: 1 / I at most max_finite / 1024
    const T edge = T(1024) / tf_max_finite(T(0));          // its inverse is max / 1024 up to rounding: take a step to either side
    CHECK(plan_on<T>(true, true, false, 0, 1, edge * T(2), edge * T(2), edge * T(2), h) == 1, "%s: 1/I = max/2048 must be on", Name<T>::s());
    CHECK(plan_on<T>(true, true, false, 0, 1, edge / T(2), edge * T(2), edge * T(2), h) == 0, "%s: 1/I = max/512 must be off", Name<T>::s());
    CHECK(plan_on<T>(true, true, false, 0, 1, inf, inf, inf, h) == 1, "%s: I = inf (1/I = 0) must be on", Name<T>::s());
    for (T hb : { T(0), -T(0), -h, inf, -inf, nan })
        CHECK(plan_on<T>(true, true, false, 2, 1, 1, 1, 1, hb) == 0, "%s: h = %g must be off", Name<T>::s(), (double)hb);
    printf("%s truth table: %s\n", Name<T>::s(), failures == before ? "ok" : "FAILED");
}

template <class T> static void constants()
{
    const int before = failures;
    Rng r{ 77 };
    const T special[] = { T(1), T(0), -T(0), T(0.5), T(3), denormal<T>(), Limits<T>::inf(), Limits<T>::nan(), (T)1e19, (T)3e38, T(-2.5) };
    const int ns = (int)(sizeof(special) / sizeof(special[0]));
    for (int it = 0; it < 20000; it++) {
        const T m = it % 3 == 0 ? special[r.next() % ns] : (T)(0.01 + 10.0 * r.uni());
        const T h = it % 5 == 0 ? special[r.next() % ns] : (T)(1e-4 + 0.1 * r.uni());
        T g[3], Ib[3] = { 1, 1, 1 };
        for (int k = 0; k < 3; k++) g[k] = it % 7 == 0 ? special[r.next() % ns] : (T)r.sym(20.0);
        const TorqueFree<T> tf = torque_free_plan<T>(true, true, false, 0, m, Ib, h, g);
        // as tick_tail and tick_head spell them
        const T invMass = T(1) / m;
        const T hm = h * invMass;
        CHECK(bits(tf.hm) == bits(hm), "%s: hm of h = %g, m = %g", Name<T>::s(), (double)h, (double)m);
        for (int k = 0; k < 3; k++) {
            T facc = T(0);
            facc = fma_(m, g[k], facc);
            CHECK(bits(tf.mg[k]) == bits(facc), "%s: mg[%d] of m = %g, g = %g", Name<T>::s(), k, (double)m, (double)g[k]);
        }
    }
    printf("%s constants: %s\n", Name<T>::s(), failures == before ? "ok" : "FAILED");
}

// the general tick of a body without rows, force accumulators or gyroscopic torque: dmx_step_fused.hpp's tick_head and tick_tail
// restated statement by statement (the gyroscopic torque is what the rule excludes)
template <class T>
static void general_tick(V3<T> &x, Q4<T> &q, V3<T> &v, V3<T> &w, T mass, const V3<T> &Ib, const V3<T> &g, T h)
{
    V3<T> facc = { T(0), T(0), T(0) }, tacc = { T(0), T(0), T(0) };
    const M3<T> R = quat_to_R(q);
    const V3<T> invIb = { T(1) / Ib.x, T(1) / Ib.y, T(1) / Ib.z };
    facc.x = fma_(mass, g.x, facc.x); facc.y = fma_(mass, g.y, facc.y); facc.z = fma_(mass, g.z, facc.z);
    const M3<T> invIw = rotate_diag(R, invIb);
    const T invMass = T(1) / mass;
    const T hm = h * invMass;
    v.x = fma_(hm, facc.x, v.x); v.y = fma_(hm, facc.y, v.y); v.z = fma_(hm, facc.z, v.z);
    tacc.x *= h; tacc.y *= h; tacc.z *= h;
    const V3<T> dw = mulv(invIw, tacc);
    w.x += dw.x; w.y += dw.y; w.z += dw.z;
    x.x = fma_(h, v.x, x.x); x.y = fma_(h, v.y, x.y); x.z = fma_(h, v.z, x.z);
    integrate_quat(q, w, h);
}

template <class T> static void ticks(int64_t n)
{
    const int before = failures;
    Rng r{ sizeof(T) == 4 ? 2024u : 4048u };
    const T inf = Limits<T>::inf();
    const T special[] = { T(0), -T(0), denormal<T>(), -denormal<T>(), inf, -inf, Limits<T>::nan(), snan<T>(), (T)1e19, (T)-1e19, (T)3e38, (T)-3e38 };
    const int ns = (int)(sizeof(special) / sizeof(special[0]));
    // launches: uniform constants the rule admits -- unit, anisotropic (gyro 0), heavy, and inverse inertias near the rule's bound
    struct Launch { T m, I[3], h, g[3]; };
    const T edge = T(2048) / tf_max_finite(T(0));
    const Launch launches[] = {
        { 1, { 1, 1, 1 }, T(1) / T(60), { 0, T(-9.81), 0 } },
        { T(2.5), { T(0.4), T(1.7), T(3.1) }, T(0.01), { T(0.3), T(-9.81), T(-1.1) } },
        { T(1e-3), { edge, T(1), edge * T(3) }, T(1) / T(240), { 0, 0, T(-1.62) } },
        { T(40), { T(1e6), T(2e6), T(1e-6) }, T(0.1), { 0, -0.0f, 0 } },
    };
    int64_t admitted = 0, rejected = 0, rejected_differ = 0, differ = 0;
    for (int64_t i = 0; i < n; i++) {
        const Launch &L = launches[i & 3];
        const V3<T> Ib = { L.I[0], L.I[1], L.I[2] }, g = { L.g[0], L.g[1], L.g[2] };
        const TorqueFree<T> tf = torque_free_plan<T>(true, true, false, 0, L.m, L.I, L.h, L.g);
        if (i < 4) CHECK(tf.on == 1, "%s: launch %d must be admitted by the rule", Name<T>::s(), (int)i);
        T c[13];
        for (int k = 0; k < 3; k++) c[k] = (T)r.sym(100.0);
        double qn = 0, qq[4];
        for (int k = 0; k < 4; k++) { qq[k] = r.sym(1.0); qn += qq[k] * qq[k]; }
        const double scale = (i & 15) == 5 ? 1.0 + r.uni() : 1.0;          // some not normalised, up to |q.k| < 2
        for (int k = 0; k < 4; k++) c[3 + k] = (T)(qq[k] / (qn > 0 ? __builtin_sqrt(qn) : 1.0) * scale);
        for (int k = 0; k < 3; k++) c[7 + k] = (T)r.sym(10.0);
        for (int k = 0; k < 3; k++) c[10 + k] = (T)r.sym(30.0);
        if ((i & 3) == 3) {                                                // a quarter of them: special values planted
            const int np = 1 + (int)(r.next() % 3);
            for (int p = 0; p < np; p++) c[r.next() % 13] = special[r.next() % ns];
        }
        if ((i & 63) == 9) c[10 + r.next() % 3] = special[r.next() % ns];  // ... and more of them in w, which the short tick keeps
        V3<T> x = { c[0], c[1], c[2] }, v = { c[7], c[8], c[9] }, w = { c[10], c[11], c[12] };
        Q4<T> q = { c[3], c[4], c[5], c[6] };
        V3<T> x2 = x, v2 = v, w2 = w;
        Q4<T> q2 = q;
        const bool admit = torque_free_admits(q);
        general_tick(x, q, v, w, L.m, Ib, g, L.h);
        torque_free_step(x2, q2, v2, w2, tf.hm, V3<T>{ tf.mg[0], tf.mg[1], tf.mg[2] }, L.h);
        const T a[13] = { x.x, x.y, x.z, q.w, q.x, q.y, q.z, v.x, v.y, v.z, w.x, w.y, w.z };
        const T b[13] = { x2.x, x2.y, x2.z, q2.w, q2.x, q2.y, q2.z, v2.x, v2.y, v2.z, w2.x, w2.y, w2.z };
        bool same = true;
        for (int k = 0; k < 13; k++) same = same && bits(a[k]) == bits(b[k]);
        if (admit) {
            admitted++;
            if (!same) {
                if (differ++ < 5)
                    for (int k = 0; k < 13; k++)
                        if (bits(a[k]) != bits(b[k]))
                            printf("  %s body %lld component %d: general %a short %a (loaded %a)\n", Name<T>::s(), (long long)i, k, (double)a[k], (double)b[k], (double)c[k]);
            }
        } else {
            rejected++;
            rejected_differ += !same;
        }
    }
    CHECK(differ == 0, "%s: %lld of %lld admitted bodies differ from the general tick", Name<T>::s(), (long long)differ, (long long)admitted);
    CHECK(admitted * 10 > n * 8, "%s: only %lld of %lld bodies admitted", Name<T>::s(), (long long)admitted, (long long)n);
    CHECK(rejected > 0 && rejected_differ > 0, "%s: no rejected body differs (%lld rejected): the planted values do not reach the guard", Name<T>::s(), (long long)rejected);
    // what the guard must reject, whatever the other components hold
    for (int k = 0; k < 4; k++) {
        T u[4] = { T(0.5), T(0.5), T(0.5), T(0.5) };
        Q4<T> ok = { u[0], u[1], u[2], u[3] };
        CHECK(torque_free_admits(ok), "%s: a unit quaternion must be admitted", Name<T>::s());
        for (T badv : { Limits<T>::nan(), snan<T>(), inf, -inf }) {
            u[k] = badv;
            const Q4<T> qb = { u[0], u[1], u[2], u[3] };
            CHECK(!torque_free_admits(qb), "%s: q[%d] = %g must be rejected", Name<T>::s(), k, (double)badv);
        }
    }
    const Q4<T> ident3 = { T(3), T(0), T(0), T(0) }, ident2 = { T(2), T(0), T(0), T(0) }, neg3 = { T(0), T(0), T(-3), T(0) };
    const Q4<T> half3 = { T(1.5), T(1.5), T(1.5), T(1.5) };       // a unit quaternion scaled by 3, every |q.k| <= 2: R finite, admitted
    const Q4<T> axis3 = { T(3) * T(0.8), T(0), T(3) * T(0.6), T(0) };
    CHECK(!torque_free_admits(ident3) && !torque_free_admits(neg3) && !torque_free_admits(axis3), "%s: a 3x scaled quaternion with a component beyond 2 must be rejected", Name<T>::s());
    CHECK(torque_free_admits(ident2) && torque_free_admits(half3), "%s: |q.k| <= 2 must be admitted", Name<T>::s());
    printf("%s ticks: %lld bodies, %lld admitted (0 may differ: %lld do), %lld rejected of which %lld differ: %s\n", Name<T>::s(), (long long)n,
           (long long)admitted, (long long)differ, (long long)rejected, (long long)rejected_differ, failures == before ? "ok" : "FAILED");
}

int main(int argc, char **argv)
{
    const int64_t n = argc > 1 ? atoll(argv[1]) : 1048576;
    truth_table<float>(); truth_table<double>();
    constants<float>(); constants<double>();
    ticks<float>(n); ticks<double>(n);
    printf(failures == 0 ? "torque_free_harness: all checks hold\n" : "torque_free_harness: %d checks FAILED\n", failures);
    return failures == 0 ? 0 : 1;
}
