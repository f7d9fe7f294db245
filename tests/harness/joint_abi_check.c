/* tests/harness/joint_abi_check.c -- a plain C99 client of include/dmx_batch.h: prints the layout of dmxJoint (every field's
 * offset and the struct's size), which tests/test_joint_reference.py compares with batch.JOINT_DTYPE, and takes the address of
 * the articulation joints' entry points so that the link fails if one is missing.  Needs no HIP device. */
#include <stdio.h>
#include <stddef.h>
#include "dmx_batch.h"

int main(void)
{
    int (*set_joints)(dmxBatchID, int64_t, const dmxJoint *) = dmxBatchSetJoints;
    int64_t (*count)(dmxBatchID) = dmxBatchJointCount;
    int (*from_world)(dmxBatchID, int, int32_t, int32_t, const double *, const double *, dmxJoint *) = dmxBatchJointFromWorld;
    int (*errors)(dmxBatchID, double *, double *, double *) = dmxBatchJointErrors;
    printf("kind %zu\n", offsetof(dmxJoint, kind));
    printf("body1 %zu\n", offsetof(dmxJoint, body1));
    printf("body2 %zu\n", offsetof(dmxJoint, body2));
    printf("reserved %zu\n", offsetof(dmxJoint, reserved));
    printf("anchor1 %zu\n", offsetof(dmxJoint, anchor1));
    printf("anchor2 %zu\n", offsetof(dmxJoint, anchor2));
    printf("axis1 %zu\n", offsetof(dmxJoint, axis1));
    printf("axis2 %zu\n", offsetof(dmxJoint, axis2));
    printf("sizeof %zu\n", sizeof(dmxJoint));
    printf("DMX_JOINT_BALL %d\nDMX_JOINT_HINGE %d\n", DMX_JOINT_BALL, DMX_JOINT_HINGE);
    /* a null batch is refused by every one of them (no device touched) */
    return (set_joints(NULL, 0, NULL) != DMX_OK && count(NULL) < 0 && from_world(NULL, 1, 0, 0, NULL, NULL, NULL) != DMX_OK &&
            errors(NULL, NULL, NULL, NULL) != DMX_OK) ? 0 : 1;
}
