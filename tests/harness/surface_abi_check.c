/* tests/harness/surface_abi_check.c -- a plain C99 client of include/dmx_batch.h and include/ode/ode.h: prints the layout of
 * dmxContactSurface (every field's offset and the struct's size) and of dmxContactJoint (its size: the struct is ABI and does not
 * change), which tests/test_surface_abi.py checks against batch.CONTACT_SURFACE_DTYPE; holds the seven DMX_CONTACT_* bits to ODE's
 * dContact* values at compile time; and takes the address of dmxBatchStepJointsSurface, so that the link fails if it is missing or
 * the compile if its signature differs (compile with -DdSINGLE or -DdDOUBLE for the two libraries).  Needs no HIP device. */
#include <stdio.h>
#include <stddef.h>
#include "dmx_batch.h"
#include "ode/ode.h"

typedef char same_mu2[(int)DMX_CONTACT_MU2 == (int)dContactMu2 ? 1 : -1];
typedef char same_fdir1[(int)DMX_CONTACT_FDIR1 == (int)dContactFDir1 ? 1 : -1];
typedef char same_motion1[(int)DMX_CONTACT_MOTION1 == (int)dContactMotion1 ? 1 : -1];
typedef char same_motion2[(int)DMX_CONTACT_MOTION2 == (int)dContactMotion2 ? 1 : -1];
typedef char same_motionn[(int)DMX_CONTACT_MOTIONN == (int)dContactMotionN ? 1 : -1];
typedef char same_slip1[(int)DMX_CONTACT_SLIP1 == (int)dContactSlip1 ? 1 : -1];
typedef char same_slip2[(int)DMX_CONTACT_SLIP2 == (int)dContactSlip2 ? 1 : -1];
typedef char ext_is_the_seven[(int)DMX_CONTACT_SURFACE_EXT == (dContactMu2 | dContactFDir1 | dContactMotion1 | dContactMotion2 | dContactMotionN |
                                                              dContactSlip1 | dContactSlip2) ? 1 : -1];

int main(void)
{
    int (*step)(dmxBatchID, double, int64_t, const dmxContactJoint *, const dmxContactSurface *) = dmxBatchStepJointsSurface;
    dmxContactSurface s;
    printf("mu2 %zu\nfdir1 %zu\nmotion1 %zu\nmotion2 %zu\nmotionN %zu\nslip1 %zu\nslip2 %zu\nsizeof %zu\njoint %zu\next %d\n",
           offsetof(dmxContactSurface, mu2), offsetof(dmxContactSurface, fdir1), offsetof(dmxContactSurface, motion1),
           offsetof(dmxContactSurface, motion2), offsetof(dmxContactSurface, motionN), offsetof(dmxContactSurface, slip1),
           offsetof(dmxContactSurface, slip2), sizeof(dmxContactSurface), sizeof(dmxContactJoint), (int)DMX_CONTACT_SURFACE_EXT);
    /* a null batch is refused, with surfaces and without (no device touched) */
    s.mu2 = 0;
    return (step(NULL, 0.01, 0, NULL, &s) != DMX_OK && step(NULL, 0.01, 0, NULL, NULL) != DMX_OK) ? 0 : 1;
}
