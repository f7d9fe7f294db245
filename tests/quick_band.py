"""The band float32 QuickStep is held to against the dense float64 reference (tests/lcp_dense.py), clamps included.

Test infrastructure, not a test file.  Pure numpy, float64 except inside `emulate_f32`; it shares no code with csrc/ or oracle/.

The model.  For an island I of the reference (any class derived from lcp_dense.Island) with the reference's lambda, per
velocity component

    M_v = |v| + h |M^-1 f| + h (|M^-1 J^T| . |lambda|)                                  (absolute values entry by entry)

the sum of the magnitudes of the terms whose sum is v' -- impulses that cancel still count.  A body's M_v is the largest of its
six components.  The bands:

    velocity      K eps32 M_v(body)
    position      h x the velocity band + 4 eps32 max(1, |pos|)
    quaternion    h x the velocity band + 4 eps32

No clamp-margin gate goes with it: the projection onto [lo, hi] is non-expansive, so a decision that rounding flips next to a
bound moves lambda by no more than the rounding did (tests/test_quick_band.py holds that on the cases the old gate refused).

K is derived, not fitted: measured on the CPU over two populations per family -- (a) the float32
oracle's one-tick deviation from the reference built from its own float32 pre-tick state, (b) a float32 emulation of the
reference's own sweeps (`emulate_f32`) on the inputs of every GPU case held to the band -- then K = 2 x the largest value,
rounded up to a power of two.  A family that needs K above K_MAX is missing a factor in the model: a finding, never a reason
to raise K.  The device's own output never enters K.  tests/test_quick_band.py re-measures both populations and asserts the
table below."""
import numpy as np

import lcp_dense as ld

EPS32 = float(np.finfo(np.float32).eps)
K_MAX = 64

# the largest deviation measured on the CPU, in units of eps32 M_v(body), per family and population (tests/test_quick_band.py
# prints them); "oracle": population (a), "emulation": population (b)
MEASURED = {
    # contact rows (tests/test_gpu_solver_dense.py, test_gpu_small_tick.py, test_gpu_body_flags.py)
    "contact": {"oracle": 5.31, "emulation": 3.76},
}
# Islands with joint rows are not held to the band, and have no K.  The float32 sweeps alone deviate by "sweeps" over the float32
# QuickStep cases of test_gpu_joints.py, test_gpu_hinge_limot.py and test_gpu_slider.py; with R anchor and R axis of the rows
# evaluated in float32 too by "rows", above K_MAX / 2: the right-hand sides carry (ERP / h) eps32 |R anchor|, a term M_v lacks
# (tests/test_quick_band.py::test_joint_rows_need_a_term_the_model_lacks).  Those files keep 10 eps32 kappa(A)
JOINT_MEASURED = {"sweeps": 3.78, "rows": 35.37}


def k_rule(worst):
    """the K_BAND rule: 2 x the largest measured value, rounded up to a power of two"""
    return int(2 ** int(np.ceil(np.log2(2.0 * worst))))


K = {family: k_rule(max(m.values())) for family, m in MEASURED.items()}


# ---------------------------------------------------------------------------------------------------------------------
def condition_model(I, lam):
    """M_v of every velocity component of island I (6 per body, in the island's body order)"""
    nb = len(I.Mblk)
    mv = np.abs(I.v) + I.h * np.abs(I.minv(I.f))
    if I.m:
        # |M^-1 J^T| |lambda|: M^-1 is block diagonal, so one 6 x 6 block times the body's six columns of J
        MJ = np.abs(np.einsum("kij,rkj->rki", I.Mblk, I.J.reshape(I.m, nb, 6)))           # (m, nb, 6)
        mv = mv + I.h * np.einsum("rki,r->ki", MJ, np.abs(lam)).reshape(-1)
    return mv


def body_model(I, lam):
    """M_v per body of the island: the largest of its six components"""
    return condition_model(I, lam).reshape(-1, 6).max(axis=1)


def emulate_f32(I, iters, w):
    """the reference's own sweeps (Island.quickstep) with A, b, lo, hi cast to float32 and the same loop, w and iters in
    float32 -> lambda (float32).  Row i's update is lambda_i + w (b_i - A_i . lambda) / A_ii, every operation rounded"""
    f = np.float32
    A, b, lo, hi = I.A.astype(f), I.b.astype(f), I.lo.astype(f), I.hi.astype(f)
    w = f(w)
    lam = np.zeros(I.m, f)
    d = np.diag(A).copy()
    for _ in range(iters):
        for i in range(I.m):
            x = lam[i] + w * (b[i] - A[i] @ lam) / d[i]
            lam[i] = min(max(x, lo[i]), hi[i])
    return lam


def model_per_slot(result):
    """M_v of every body slot over all islands of a Result (0 for slots in no island: dead ones)"""
    if getattr(result, "_mv_slots", None) is None:
        out = np.zeros(result.bodies.n)
        for I, lam in zip(result.islands, result.lams):
            out[np.asarray(I.slots, int)] = body_model(I, lam)
        result._mv_slots = out
    return result._mv_slots


def velocity_band(result, world, K):
    """K eps32 M_v per body slot, over all islands of `result` (a lcp_dense.Result or one with .islands / .lams / .bodies);
    `world` is part of the signature for a model that needs h or ERP per world -- M_v takes h from the islands"""
    return K * EPS32 * model_per_slot(result)


def deviation(result, lvel, avel):
    """per body slot, the largest |v - v_ref| of its six components in units of eps32 M_v(body)"""
    d = np.maximum(np.max(np.abs(np.asarray(lvel, np.float64) - result.bodies.lvel), axis=1),
                   np.max(np.abs(np.asarray(avel, np.float64) - result.bodies.avel), axis=1))
    mv = model_per_slot(result)
    out = np.zeros(len(d))
    nz = mv > 0
    out[nz] = d[nz] / (EPS32 * mv[nz])
    out[~nz & (d > 0)] = np.inf
    return out


def emulation_deviation(result, world):
    """population (b) on the islands of a reference Result: the float32 sweeps' velocities against the reference's own, per
    body slot in units of eps32 M_v"""
    out = np.zeros(result.bodies.n)
    for I, lam in zip(result.islands, result.lams):
        if not I.m:
            continue
        dv = np.abs(I.velocities(emulate_f32(I, world.iters, world.sor_w).astype(np.float64)) - I.velocities(lam))
        out[np.asarray(I.slots, int)] = dv.reshape(-1, 6).max(axis=1) / (EPS32 * body_model(I, lam))
    return out


def assert_in_band(result, world, post, K, live=None, what="float32 QuickStep"):
    """the device's (or the oracle's) post-tick state (n, 13: pos, quat, lvel, avel) against the reference Result within the
    bands of this module, per body.  -> the largest velocity deviation in units of eps32 M_v"""
    post = np.asarray(post, np.float64)
    n = result.bodies.n
    live = np.arange(n) if live is None else np.asarray(live, int)
    band = velocity_band(result, world, K)
    dev = deviation(result, post[:, 7:10], post[:, 10:13])
    worst = float(np.max(dev[live], initial=0.0))
    dv = np.maximum(np.max(np.abs(post[:, 7:10] - result.bodies.lvel), axis=1), np.max(np.abs(post[:, 10:13] - result.bodies.avel), axis=1))
    bad = live[dv[live] > band[live]]
    assert len(bad) == 0, (f"{what}: velocity of slot {bad[0]} off by {dv[bad[0]]:.3e} = {dev[bad[0]]:.2f} eps32 M_v, "
                           f"band K = {K} ({len(bad)} of {len(live)} bodies out; worst {worst:.2f})")
    pmax = max(1.0, np.max(np.abs(result.bodies.pos[live]), initial=0.0))
    dx = np.max(np.abs(post[:, 0:3] - result.bodies.pos), axis=1)
    bad = live[dx[live] > world.h * band[live] + 4 * EPS32 * pmax]
    assert len(bad) == 0, f"{what}: position of slot {bad[0]} off by {dx[bad[0]]:.3e}"
    dq = np.max(np.abs(post[:, 3:7] - result.bodies.quat), axis=1)
    bad = live[dq[live] > world.h * band[live] + 4 * EPS32]
    assert len(bad) == 0, f"{what}: quaternion of slot {bad[0]} off by {dq[bad[0]]:.3e}"
    return worst


def row_margins(I, iters, w):
    """the float64 sweeps of Island.quickstep again, keeping per row the smallest distance of its updates from a finite bound
    (inf for a row without one) -> (lambda, margins)"""
    lam = np.zeros(I.m)
    margins = np.full(I.m, np.inf)
    A, b, lo, hi = I.A, I.b, I.lo, I.hi
    for _ in range(iters):
        for i in range(I.m):
            x = lam[i] + w * (b[i] - A[i] @ lam) / A[i, i]
            for bound in (lo[i], hi[i]):
                if np.isfinite(bound):
                    margins[i] = min(margins[i], abs(x - bound))
            lam[i] = min(max(x, lo[i]), hi[i])
    return lam, margins


def gate_passes(result):
    """the rule this band replaces: every island's smallest clamp margin above 1e-3 of its largest |lambda|"""
    return all(margin > 1e-3 * np.max(np.abs(lam)) for I, lam, margin in zip(result.islands, result.lams, result.margins) if I.m)


def as_f32_inputs(B, W, jts):
    """(Bodies, World, joints) as a float32 batch holds them, in float64: the device's pre-tick state is bit for bit these"""
    r = lambda x: np.asarray(x, np.float64).astype(np.float32).astype(np.float64)
    B2 = ld.Bodies(r(B.pos), r(B.quat), r(B.lvel), r(B.avel), r(B.mass), r(B.inertia), B.flags)
    W2 = ld.World(h=float(r(W.h)), gravity=r(W.gravity), erp=float(r(W.erp)), cfm=float(r(W.cfm)), iters=W.iters,
                  sor_w=float(r(W.sor_w)), gyro=W.gyro)
    j2 = jts.copy()
    for f in ("pos", "normal", "depth", "mu", "bounce", "bounce_vel", "soft_erp", "soft_cfm"):
        j2[f] = r(jts[f])
    return B2, W2, j2
