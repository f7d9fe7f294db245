/* tests/harness/feedback_abi_check.c -- a plain C99 client of include/dmx_batch.h and include/ode/ode.h: prints the layout of
 * dmxJointFeedback and of dJointFeedback (every field's offset and the structs' sizes; compile with -DdSINGLE or -DdDOUBLE for the
 * two widths of dReal), which tests/test_feedback_reference.py checks, and takes the address of the feedback entry points so that
 * the link fails if one is missing.  Needs no HIP device. */
#include <stdio.h>
#include <stddef.h>
#include "dmx_batch.h"
#include "ode/ode.h"

int main(void)
{
    int (*set)(dmxBatchID, int) = dmxBatchSetFeedback;
    int (*joints)(dmxBatchID, dmxJointFeedback *) = dmxBatchJointFeedback;
    int (*contacts)(dmxBatchID, int64_t, dmxJointFeedback *) = dmxBatchContactFeedback;
    int (*device)(dmxBatchID, const void **, const void **) = dmxBatchFeedbackDevice;
    void (*ode_set)(dJointID, dJointFeedback *) = dJointSetFeedback;
    dJointFeedback *(*ode_get)(dJointID) = dJointGetFeedback;
    printf("dmx.f1 %zu\ndmx.t1 %zu\ndmx.f2 %zu\ndmx.t2 %zu\ndmx.sizeof %zu\n", offsetof(dmxJointFeedback, f1), offsetof(dmxJointFeedback, t1),
           offsetof(dmxJointFeedback, f2), offsetof(dmxJointFeedback, t2), sizeof(dmxJointFeedback));
    printf("ode.f1 %zu\node.t1 %zu\node.f2 %zu\node.t2 %zu\node.sizeof %zu\n", offsetof(dJointFeedback, f1), offsetof(dJointFeedback, t1),
           offsetof(dJointFeedback, f2), offsetof(dJointFeedback, t2), sizeof(dJointFeedback));
    printf("dReal %zu\n", sizeof(dReal));
    /* a null batch or joint is refused by every one of them (no device touched) */
    ode_set(NULL, NULL);
    return (set(NULL, 1) != DMX_OK && joints(NULL, NULL) != DMX_OK && contacts(NULL, 0, NULL) != DMX_OK && device(NULL, NULL, NULL) != DMX_OK &&
            ode_get(NULL) == NULL) ? 0 : 1;
}
