// dmx_uniform.hpp -- does every slot of the batch hold the same value in a constant field (mass, inertia)?
//
// Host side only, no HIP: the rule is tested on the CPU (tests/test_uniform_tracker.py).  Constants enter the slab
// through one door, dmxBatchUpload (dmx_batch.cpp: upload_t), from a host array, so the host can know for nothing
// when a field is the same for all n slots; integrate_free then takes it as a kernel argument instead of loading it
// per body (StepParams::uni).  The tracker is conservative: it may say "mixed" while the slots happen to be equal,
// never "uniform" while they are not.
//   state        all n slots hold v (at creation: v = 1, what fill_defaults writes), or mixed
//   upload of [first, first+count), every row equal to v    -> unchanged
//   upload of [0, n), every row equal to one value u        -> uniform, v = u
//   anything else                                           -> mixed (only a full-range upload of one value leaves it)
//   poison(): somebody holds a device pointer into the slab (any dmxBatchDevicePtr) and may write the field unseen -> mixed for good
// Values are compared by their bits (-0.0 is not +0.0; a NaN is never uniform).  Pad slots [n, stride) keep their ones:
// they are inert and unobservable, so they may be stepped with v.
#pragma once
#include <stdint.h>
#include <string.h>

namespace dmx {

template <int K> struct UniformTracker {
    bool uniform = true, poisoned = false;
    double v[K];                // the common row; exact for f32 and f64 batches alike
    UniformTracker() { for (int j = 0; j < K; j++) v[j] = 1.0; }

    template <class T> static bool same_bits(T a, T b) { return memcmp(&a, &b, sizeof(T)) == 0; }

    // host = count rows of K values of the batch's precision, about to be written to slots [first, first + count) of n
    template <class T> void on_upload(const T *host, int64_t first, int64_t count, int64_t n)
    {
        if (count <= 0) return;
        bool one = true;        // every row equals row 0, and row 0 holds no NaN
        for (int j = 0; j < K; j++) one = one && host[j] == host[j];
        for (int64_t i = 1; one && i < count; i++)
            for (int j = 0; j < K; j++) one = one && same_bits(host[i * K + j], host[j]);
        if (first == 0 && count == n) {
            uniform = one && !poisoned;
            if (uniform) for (int j = 0; j < K; j++) v[j] = (double)host[j];
            return;
        }
        if (!uniform) return;
        for (int j = 0; one && j < K; j++) one = same_bits(host[j], (T)v[j]);
        uniform = one;
    }
    void poison() { uniform = false; poisoned = true; }
};

}  // namespace dmx
