// C entry points around dmx::UniformTracker (csrc/dmx_uniform.hpp) for tests/test_uniform_tracker.py: plain g++, no HIP.
#include "dmx_uniform.hpp"

template <int K, class T> struct Box { dmx::UniformTracker<K> t; };

#define TRACKER_API(NAME, K, T)                                                                                   \
    extern "C" void *NAME##_new() { return new dmx::UniformTracker<K>(); }                                        \
    extern "C" void NAME##_free(void *p) { delete (dmx::UniformTracker<K> *)p; }                                  \
    extern "C" void NAME##_upload(void *p, const T *host, int64_t first, int64_t count, int64_t n)                \
    { ((dmx::UniformTracker<K> *)p)->on_upload(host, first, count, n); }                                          \
    extern "C" void NAME##_poison(void *p) { ((dmx::UniformTracker<K> *)p)->poison(); }                           \
    extern "C" int NAME##_get(void *p, double *v)                                                                 \
    {                                                                                                             \
        const dmx::UniformTracker<K> *t = (const dmx::UniformTracker<K> *)p;                                      \
        for (int j = 0; j < K; j++) v[j] = t->v[j];                                                               \
        return t->uniform ? 1 : 0;                                                                                \
    }
TRACKER_API(ut1f, 1, float)
TRACKER_API(ut3f, 3, float)
TRACKER_API(ut1d, 1, double)
TRACKER_API(ut3d, 3, double)
