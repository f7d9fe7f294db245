// dmx_damping.hip -- the start-of-tick damping pass of dmxBatchStepJoints: damp_body (dmx_damping.hpp) for every slot the tick
// steps, a lane each, in front of the tick's first kernel on the batch's stream -- the general path's kernels or the single-launch
// tick's one launch, whose body list it reads where that launch reads it.  Launched only while some slot's scale is not zero.
#include <hip/hip_runtime.h>
#include "dmx_damping.hpp"

namespace dmx {

template <class T>
__global__ __launch_bounds__(256) void damping_apply(T *S, const uint8_t *flags, const T *table, const int *bodies, int n_bodies, int n_slots)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n_bodies) return;
    const int s = bodies[i];
    if (s < 0 || s >= n_slots) return;
    damp_body<T>(S, flags, table, s);
}

template <class T>
hipError_t launch_damping(T *S, const uint8_t *flags, const T *table, const int *bodies, int n_bodies, int n_slots, hipStream_t st)
{
    if (n_bodies <= 0) return hipSuccess;
    hipLaunchKernelGGL((damping_apply<T>), dim3((unsigned)((n_bodies + 255) / 256)), dim3(256), 0, st, S, flags, table, bodies, n_bodies, n_slots);
    return hipGetLastError();
}
template hipError_t launch_damping<float>(float *, const uint8_t *, const float *, const int *, int, int, hipStream_t);
template hipError_t launch_damping<double>(double *, const uint8_t *, const double *, const int *, int, int, hipStream_t);

}  // namespace dmx
