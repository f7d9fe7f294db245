/* tests/harness/limot_abi_check.c -- a plain C99 client of include/dmx_batch.h: prints the layout of dmxHingeLimot (every field's
 * offset and the struct's size), which tests/test_limot_reference.py compares with batch.HINGE_LIMOT_DTYPE, and takes the address
 * of the hinge limots' entry points so that the link fails if one is missing.  Needs no HIP device. */
#include <stdio.h>
#include <stddef.h>
#include "dmx_batch.h"

int main(void)
{
    int (*set_limots)(dmxBatchID, int64_t, const dmxHingeLimot *) = dmxBatchSetHingeLimots;
    int (*init)(dmxBatchID, const dmxJoint *, dmxHingeLimot *) = dmxBatchHingeLimotInit;
    int (*angles)(dmxBatchID, double *, double *) = dmxBatchHingeAngles;
    printf("lo_stop %zu\n", offsetof(dmxHingeLimot, lo_stop));
    printf("hi_stop %zu\n", offsetof(dmxHingeLimot, hi_stop));
    printf("vel %zu\n", offsetof(dmxHingeLimot, vel));
    printf("fmax %zu\n", offsetof(dmxHingeLimot, fmax));
    printf("qrel0 %zu\n", offsetof(dmxHingeLimot, qrel0));
    printf("sizeof %zu\n", sizeof(dmxHingeLimot));
    /* a null batch is refused by every one of them (no device touched) */
    return (set_limots(NULL, 0, NULL) != DMX_OK && init(NULL, NULL, NULL) != DMX_OK && angles(NULL, NULL, NULL) != DMX_OK) ? 0 : 1;
}
