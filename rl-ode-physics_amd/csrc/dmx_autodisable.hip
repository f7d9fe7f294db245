// dmx_autodisable.hip -- the general path's end-of-tick auto-disable pass: idle_update (dmx_autodisable.hpp) for every slot the
// tick stepped, a lane each, behind the tick's last kernel on the batch's stream.  Launched only by a tick that stepped a body
// with DMX_BODY_AUTODISABLE.
#include <hip/hip_runtime.h>
#include "dmx_autodisable.hpp"

namespace dmx {

template <class T>
__global__ __launch_bounds__(256) void autodisable_update(T *S, uint8_t *flags, int32_t *steps_left, double *time_left, IdleParams<T> A,
                                                          const int *bodies, int n_bodies, int n_slots)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n_bodies) return;
    const int s = bodies[i];
    if (s < 0 || s >= n_slots) return;
    (void)idle_update<T>(S, flags, steps_left, time_left, A, s);
}

template <class T>
hipError_t launch_autodisable_update(T *S, uint8_t *flags, int32_t *steps_left, double *time_left, const IdleParams<T> &A, const int *bodies, int n_bodies,
                                     int n_slots, hipStream_t st)
{
    if (n_bodies <= 0) return hipSuccess;
    hipLaunchKernelGGL((autodisable_update<T>), dim3((unsigned)((n_bodies + 255) / 256)), dim3(256), 0, st, S, flags, steps_left, time_left, A, bodies,
                       n_bodies, n_slots);
    return hipGetLastError();
}
template hipError_t launch_autodisable_update<float>(float *, uint8_t *, int32_t *, double *, const IdleParams<float> &, const int *, int, int, hipStream_t);
template hipError_t launch_autodisable_update<double>(double *, uint8_t *, int32_t *, double *, const IdleParams<double> &, const int *, int, int, hipStream_t);

}  // namespace dmx
