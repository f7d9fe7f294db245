/* tests/harness/damping_abi_check.c -- a plain C99 client of include/dmx_batch.h and include/ode/ode.h: prints the layout of
 * dmxBodyDamping (every field's offset and the struct's size), which tests/test_stability_abi.py checks against
 * batch.BODY_DAMPING_DTYPE, and takes the address of every entry point of the damping section -- the batch's six and the ODE
 * face's (compile with -DdSINGLE or -DdDOUBLE for the two widths of dReal) -- so that the link fails if one is missing or the
 * compile if a signature differs.  Needs no HIP device. */
#include <stdio.h>
#include <stddef.h>
#include "dmx_batch.h"
#include "ode/ode.h"

int main(void)
{
    int (*set_damping)(dmxBatchID, double, double, double, double) = dmxBatchSetDamping;
    int (*set_max)(dmxBatchID, double) = dmxBatchSetMaxAngularSpeed;
    int (*upload)(dmxBatchID, const dmxBodyDamping *, int64_t, int64_t) = dmxBatchUploadBodyDamping;
    int (*download)(dmxBatchID, dmxBodyDamping *, int64_t, int64_t) = dmxBatchDownloadBodyDamping;
    int (*set_cc)(dmxBatchID, double, double) = dmxBatchSetContactCorrection;
    int (*get_cc)(dmxBatchID, double *, double *) = dmxBatchGetContactCorrection;
    void (*wset[])(dWorldID, dReal) = { dWorldSetLinearDamping, dWorldSetAngularDamping, dWorldSetLinearDampingThreshold, dWorldSetAngularDampingThreshold,
                                        dWorldSetMaxAngularSpeed, dWorldSetContactSurfaceLayer, dWorldSetContactMaxCorrectingVel };
    dReal (*wget[])(dWorldID) = { dWorldGetLinearDamping, dWorldGetAngularDamping, dWorldGetLinearDampingThreshold, dWorldGetAngularDampingThreshold,
                                  dWorldGetMaxAngularSpeed, dWorldGetContactSurfaceLayer, dWorldGetContactMaxCorrectingVel };
    void (*bset[])(dBodyID, dReal) = { dBodySetLinearDamping, dBodySetAngularDamping, dBodySetLinearDampingThreshold, dBodySetAngularDampingThreshold,
                                       dBodySetMaxAngularSpeed };
    dReal (*bget[])(dBodyID) = { dBodyGetLinearDamping, dBodyGetAngularDamping, dBodyGetLinearDampingThreshold, dBodyGetAngularDampingThreshold,
                                 dBodyGetMaxAngularSpeed };
    void (*wboth)(dWorldID, dReal, dReal) = dWorldSetDamping;
    void (*bboth)(dBodyID, dReal, dReal) = dBodySetDamping;
    void (*bdef)(dBodyID) = dBodySetDampingDefaults;
    printf("lin_scale %zu\nang_scale %zu\nlin_threshold %zu\nang_threshold %zu\nmax_angular_speed %zu\nsizeof %zu\ndReal %zu\n",
           offsetof(dmxBodyDamping, lin_scale), offsetof(dmxBodyDamping, ang_scale), offsetof(dmxBodyDamping, lin_threshold),
           offsetof(dmxBodyDamping, ang_threshold), offsetof(dmxBodyDamping, max_angular_speed), sizeof(dmxBodyDamping), sizeof(dReal));
    printf("entries %zu\n", sizeof wset / sizeof wset[0] + sizeof wget / sizeof wget[0] + sizeof bset / sizeof bset[0] + sizeof bget / sizeof bget[0] +
                            (size_t)(wboth != NULL) + (size_t)(bboth != NULL) + (size_t)(bdef != NULL));
    /* a null batch is refused by every one of the batch's calls (no device touched) */
    return (set_damping(NULL, 0, 0, 0.01, 0.01) != DMX_OK && set_max(NULL, 1) != DMX_OK && upload(NULL, NULL, 0, 0) != DMX_OK &&
            download(NULL, NULL, 0, 0) != DMX_OK && set_cc(NULL, 0, 1) != DMX_OK && get_cc(NULL, NULL, NULL) != DMX_OK) ? 0 : 1;
}
