/* tests/harness/amotor_abi_check.c -- a plain C99 client of include/dmx_batch.h and include/ode/ode.h: prints the layout of dmxAMotor
 * (every field's offset and the struct's size), which tests/test_amotor_abi.py checks against _lib.dmxAMotor and
 * batch.AMOTOR_DTYPE; holds the new enum values to ODE's at compile time; and takes the address of every new function, so that the
 * link fails if one is missing and the compile if a signature differs (compile with -DdSINGLE or -DdDOUBLE for the two libraries).
 * Needs no HIP device. */
#include <stdio.h>
#include <stddef.h>
#include "dmx_batch.h"
#include "ode/ode.h"

typedef char amotor_type[(int)dJointTypeAMotor == 9 ? 1 : -1];
typedef char amotor_modes[(int)dAMotorUser == 0 && (int)dAMotorEuler == 1 && (int)DMX_AMOTOR_USER == (int)dAMotorUser && (int)DMX_AMOTOR_EULER == (int)dAMotorEuler ? 1 : -1];
typedef char amotor_kind[(int)DMX_JOINT_AMOTOR == 5 ? 1 : -1];
typedef char param_group[(int)dParamGroup == 0x100 ? 1 : -1];
typedef char param_group1[(int)dParamLoStop1 == (int)dParamLoStop && (int)dParamFMax1 == (int)dParamFMax && (int)dParamERP1 == (int)dParamERP ? 1 : -1];
typedef char param_group2[(int)dParamLoStop2 == 0x100 + (int)dParamLoStop && (int)dParamHiStop2 == 0x100 + (int)dParamHiStop &&
                          (int)dParamVel2 == 0x100 + (int)dParamVel && (int)dParamFMax2 == 0x100 + (int)dParamFMax && (int)dParamERP2 == 0x100 + (int)dParamERP ? 1 : -1];
typedef char param_group3[(int)dParamLoStop3 == 0x200 + (int)dParamLoStop && (int)dParamHiStop3 == 0x200 + (int)dParamHiStop &&
                          (int)dParamVel3 == 0x200 + (int)dParamVel && (int)dParamFMax3 == 0x200 + (int)dParamFMax && (int)dParamERP3 == 0x200 + (int)dParamERP ? 1 : -1];

int main(void)
{
    int (*set)(dmxBatchID, int64_t, const dmxAMotor *) = dmxBatchSetAMotors;
    int (*from)(dmxBatchID, int32_t, int32_t, int, int, const int32_t[3], const double[3][3], dmxAMotor *) = dmxBatchAMotorFromWorld;
    int (*ang)(dmxBatchID, double *, double *) = dmxBatchAMotorAngles;
    dJointID (*create)(dWorldID, dJointGroupID) = dJointCreateAMotor;
    void (*set_mode)(dJointID, int) = dJointSetAMotorMode;
    int (*get_mode)(dJointID) = dJointGetAMotorMode;
    void (*set_num)(dJointID, int) = dJointSetAMotorNumAxes;
    int (*get_num)(dJointID) = dJointGetAMotorNumAxes;
    void (*set_axis)(dJointID, int, int, dReal, dReal, dReal) = dJointSetAMotorAxis;
    void (*get_axis)(dJointID, int, dVector3) = dJointGetAMotorAxis;
    int (*get_rel)(dJointID, int) = dJointGetAMotorAxisRel;
    void (*set_angle)(dJointID, int, dReal) = dJointSetAMotorAngle;
    dReal (*get_angle)(dJointID, int) = dJointGetAMotorAngle;
    dReal (*get_rate)(dJointID, int) = dJointGetAMotorAngleRate;
    void (*set_param)(dJointID, int, dReal) = dJointSetAMotorParam;
    dReal (*get_param)(dJointID, int) = dJointGetAMotorParam;
    void (*add)(dJointID, dReal, dReal, dReal) = dJointAddAMotorTorques;
    dmxAMotor m;
    dVector3 r = { 0, 0, 0, 0 };
    printf("mode %zu\nnum_axes %zu\nrel %zu\npad %zu\naxis %zu\nref1 %zu\nref2 %zu\nangle %zu\nlo_stop %zu\nhi_stop %zu\nvel %zu\nfmax %zu\nsizeof %zu\n",
           offsetof(dmxAMotor, mode), offsetof(dmxAMotor, num_axes), offsetof(dmxAMotor, rel), offsetof(dmxAMotor, pad), offsetof(dmxAMotor, axis),
           offsetof(dmxAMotor, ref1), offsetof(dmxAMotor, ref2), offsetof(dmxAMotor, angle), offsetof(dmxAMotor, lo_stop),
           offsetof(dmxAMotor, hi_stop), offsetof(dmxAMotor, vel), offsetof(dmxAMotor, fmax), sizeof(dmxAMotor));
    printf("joint %zu\nlimot %zu\ncontact %zu\n", sizeof(dmxJoint), sizeof(dmxHingeLimot), sizeof(dmxContactJoint));
    /* null handles are refused or ignored, no device touched */
    m.mode = 0;
    set_mode(NULL, dAMotorEuler); set_num(NULL, 3); set_axis(NULL, 0, 1, 1, 0, 0); get_axis(NULL, 0, r); set_angle(NULL, 0, 0);
    set_param(NULL, dParamLoStop2, 0); add(NULL, 0, 0, 0);
    if (create(NULL, NULL) != NULL || get_mode(NULL) != dAMotorUser || get_num(NULL) != 0 || get_rel(NULL, 0) != 0) return 1;
    if (get_angle(NULL, 0) != 0 || get_rate(NULL, 0) != 0 || get_param(NULL, dParamHiStop3) != 0) return 1;
    return (set(NULL, 0, NULL) != DMX_OK && from(NULL, 0, 1, 0, 1, NULL, NULL, &m) != DMX_OK && ang(NULL, NULL, NULL) != DMX_OK) ? 0 : 1;
}
