"""The band float32 QuickStep is held to against the dense float64 reference (tests/lcp_dense.py), clamps included.

Test infrastructure, not a test file.  Pure numpy, float64 except inside `emulate_f32` and `float32_rows`; it shares no code with
csrc/ or oracle/.

The model.  For an island I of the reference (any class derived from lcp_dense.Island) with the reference's lambda, per
velocity component

    M_v = |v| + h |M^-1 f| + h (|M^-1 J^T| . |lambda|)                                  (absolute values entry by entry)

the sum of the magnitudes of the terms whose sum is v' -- impulses that cancel still count.  A body's M_v is the largest of its
six components.  A joint row counts with |lambda_i| + (ERP / h) S_i / (h A_ii): its right-hand side is ERP / h times an error
whose inputs -- R anchor, R axis, a quaternion product, an angle -- a float32 batch has rounded whatever lambda is; S_i is the
sum of their magnitudes (`joint_scales`, `attach_joint_term`).  Contact rows have no such term: a depth is an input.  The bands:

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
import contextlib

import numpy as np

import joint_dense as jd
import lcp_dense as ld
import limot_dense as lm
import slider_dense as sd

EPS32 = float(np.finfo(np.float32).eps)
K_MAX = 64

# the largest deviation measured on the CPU, in units of eps32 M_v(body), per family and population (tests/test_quick_band.py
# prints them); "oracle": population (a), "emulation": population (b)
MEASURED = {
    # contact rows (tests/test_gpu_solver_dense.py, test_gpu_small_tick.py, test_gpu_body_flags.py)
    "contact": {"oracle": 5.31, "emulation": 3.76},
    # islands with joint rows (tests/test_gpu_joints.py, test_gpu_hinge_limot.py, test_gpu_slider.py), M_v with the joint rows'
    # term (attach_joint_term); the oracle has no joints, so population (b) alone: everything a float32 batch computes for a joint
    # row in float32 (float32_rows, round_rows), then the float32 sweeps
    "joint": {"emulation": 2.91},
}
# The record of why the joint term exists: M_v WITHOUT it, over the 36 float32 QuickStep cases those files had before the band.  The
# float32 sweeps alone deviate by "sweeps"; with R anchor and R axis of the rows evaluated in float32 too by "rows", above
# K_MAX / 2: the right-hand sides carry (ERP / h) eps32 |R anchor| whatever lambda is
# (tests/test_quick_band.py::test_joint_rows_need_a_term_the_model_lacks)
JOINT_MEASURED = {"sweeps": 3.78, "rows": 35.37}


def k_rule(worst):
    """the K_BAND rule: 2 x the largest measured value, rounded up to a power of two"""
    return int(2 ** int(np.ceil(np.log2(2.0 * worst))))


K = {family: k_rule(max(m.values())) for family, m in MEASURED.items()}


# ---------------------------------------------------------------------------------------------------------------------
def condition_model(I, lam, joint_term=True):
    """M_v of every velocity component of island I (6 per body, in the island's body order).  joint_term: rows with a c_round
    (attach_joint_term) count with |lambda_i| + c_round_i / (h A_ii); False gives the model as it was before that term"""
    nb = len(I.Mblk)
    mv = np.abs(I.v) + I.h * np.abs(I.minv(I.f))
    if I.m:
        al = np.abs(lam)
        cr = getattr(I, "c_round", None)
        if joint_term and cr is not None:
            al = al + cr / (I.h * np.diag(I.A))
        # |M^-1 J^T| |lambda|: M^-1 is block diagonal, so one 6 x 6 block times the body's six columns of J
        MJ = np.abs(np.einsum("kij,rkj->rki", I.Mblk, I.J.reshape(I.m, nb, 6)))           # (m, nb, 6)
        mv = mv + I.h * np.einsum("rki,r->ki", MJ, al).reshape(-1)
    return mv


def body_model(I, lam, joint_term=True):
    """M_v per body of the island: the largest of its six components"""
    return condition_model(I, lam, joint_term).reshape(-1, 6).max(axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# The joint rows' term.  A joint row's right-hand side is c_i = (ERP / h) x an error formed from numbers the device rounds: the
# arms a = R anchor, the axes R axis, the lock's quaternion product, a limot's angle or position.  Their rounding is there
# whatever lambda is, so c_i carries eps32 (ERP / h) S_i, S_i = the sum of the magnitudes of those rounded inputs, and lambda_i
# carries that over h A_ii (b = c / h - ..., one row's update divides by A_ii).  S is taken per joint and shared by the rows of a
# unit: a ball row along a has a x d = 0 and still carries all of eps32 |a|.  x_2 - x_1 is formed by the device's diff_of_sums
# and contributes an ulp of the error itself, which is the |err| below.  (DESIGN.md section 5 has the derivation.)
def _quat_products(a):
    """how many products of two rounded unit quaternions e = conj(q_1) q_2 conj(q_0) takes for the sides as given: a world side is
    the identity and its product exact"""
    return (1 if int(a["body1"]) >= 0 and int(a["body2"]) >= 0 else 0) + 1


def joint_scales(bodies, world, a, l, b1, b2, swapped):
    """S_i of every row of one active joint in canonical sides, in slider_dense.Island's row order.  Float64, from the reference's own
    definitions (call it outside float32_rows)"""
    kind = int(a["kind"])
    x1, a1, u, x2, a2 = sd.canonical_sides(bodies, b1, b2, a, swapped)
    n1, n2 = np.linalg.norm(a1), np.linalg.norm(a2)                    # (a world side: a = 0, its anchor is a float32 input, exact)
    err = np.linalg.norm((x2 + a2) - (x1 + a1))
    s_ball = n1 + n2 + err                                              # a_1, a_2 and the compensated difference's own ulp
    nq = _quat_products(a)

    def limot(x, extra):
        # c = -k (x - stop) on the table's lines 0, 1, 2 only: a motor's c is its vel, an input
        _, _, _, line, _ = lm.row_values(x, l, world)
        if line > 2:
            return 0.0
        stop = float(l["hi_stop"]) if line == 2 else float(l["lo_stop"])
        return extra + abs(x) + abs(x - stop)

    if kind == sd.BALL:
        return [s_ball] * 3
    if kind == sd.HINGE:
        w = jd.side(bodies, b2, a["anchor1" if swapped else "anchor2"], a["axis1" if swapped else "axis2"])[2]
        # (u x w) . r: u = R_1 axis1 and w = R_2 axis2 are rounded where the side is a body, and each product of the cross product
        # is rounded at its own size |u| |w| however small the difference is
        s_hinge = ((1 if b1 >= 0 else 0) + (1 if b2 >= 0 else 0) + 1) * np.linalg.norm(u) * np.linalg.norm(w)
        out = [s_ball] * 3 + [s_hinge] * 2
        if lm.present(l):
            # theta = -2 atan2(e_v . axis1, e_w): twice the rounding of e, a unit quaternion from nq products, then theta's own
            out.append(limot(lm.angle(bodies, a, l), 2.0 * nq))
        return out
    # Phi = R_1 (2 e_v): twice the rounding of e, and the rotation's own at the size of Phi
    q0 = l["qrel0"]
    ev2, R1 = sd.lock_error(bodies, b1, b2, lm.qconj(q0) if swapped else np.asarray(q0))
    s_lock = 2.0 * nq + np.linalg.norm(R1 @ ev2)
    if kind == sd.FIXED:
        return [s_ball] * 3 + [s_lock] * 3
    if kind == sd.SLIDER:
        # (p_2 - p_1) . r with r from the rounded u: the arms, and the error once for its own ulp and once for r's
        out = [s_lock] * 3 + [n1 + n2 + 2.0 * err] * 2
        if lm.present(l):
            out.append(limot(sd.position(bodies, a), n1 + n2 + 2.0 * err))
        return out
    raise ValueError(f"joint kind {kind}")


def attach_joint_term(result, bodies, world, jts, art, lim=None):
    """give every island of `result` -- the reference's tick of (bodies, world, jts, art, lim) -- its rows' c_round = (erp / h) S_i,
    0 for contact rows.  -> result"""
    if art is None or len(art) == 0:
        return result
    if lim is None or len(lim) == 0:
        lim = sd.default_limots(len(art))           # (no limot is present, and every zero pose is the identity)
    jts = np.asarray(jts, ld.JOINT_DTYPE) if len(jts) else np.zeros(0, ld.JOINT_DTYPE)
    members = jd.canonical_arts(bodies, art) + ld.canonical(bodies, jts)
    k = world.erp / world.h
    for I, (slots, ms) in zip(result.islands, ld.islands(bodies, members)):
        assert list(slots) == list(I.slots)
        S = []
        for c in ms:
            if isinstance(c[0], tuple):
                (_, j), b1, b2, swapped = c
                S += joint_scales(bodies, world, art[j], lim[j], b1, b2, swapped)
        assert len(S) == getattr(I, "n_art_rows", 0), (len(S), getattr(I, "n_art_rows", 0))
        I.c_round = np.concatenate([k * np.array(S, np.float64), np.zeros(I.m - len(S))])
    result._mv_slots = None
    return result


# ---- a float32 batch's joint rows, emulated: everything the device computes for a joint row from its float32 inputs -- R anchor
# and R axis, the lock's quaternion product and R_1 (2 e_v), the limots' angle and position -- in float32; `round_rows` then
# rounds the rows' J and c (plane_space and the cross products, formed in float64 from those float32 values, to float32)
F32 = np.float32


def _R32(q):
    q = np.asarray(q, F32)
    w, x, y, z = (q / np.sqrt(np.sum(q * q, dtype=F32))).astype(F32)
    one, two = F32(1), F32(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
                     [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                     [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]], F32)


def _side_f32(bodies, s, anchor, axis):
    """joint_dense.side with the body's rotation, R anchor and R axis evaluated in float32 (the quaternion, the anchor and the axis
    are float32 numbers already): what a float32 batch can know of a_i = R_i anchor_i"""
    if s < 0:
        return np.array(anchor, np.float64), np.zeros(3), np.array(axis, np.float64)
    R = _R32(bodies.quat[s])
    return bodies.pos[s], (R @ np.asarray(anchor, F32)).astype(np.float64), (R @ np.asarray(axis, F32)).astype(np.float64)


def _qmul32(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]], F32)


def _pose_error32(q1, q2, q0):
    return _qmul32(_qmul32(lm.qconj(np.asarray(q1, F32)), q2), lm.qconj(np.asarray(q0, F32)))


def _angle_of_f32(q1, q2, q0, axis1):
    e = _pose_error32(q1, q2, q0)
    ax = np.asarray(axis1, F32)
    s, c = e[1] * ax[0] + e[2] * ax[1] + e[3] * ax[2], e[0]
    if c < 0:
        s, c = -s, -c
    return float(-(F32(2) * np.arctan2(F32(s), F32(c))))


def _lock_error_f32(bodies, b1, b2, q0c):
    q1 = bodies.quat[b1] if b1 >= 0 else lm.IDENT
    q2 = bodies.quat[b2] if b2 >= 0 else lm.IDENT
    e = _pose_error32(q1, q2, q0c)
    if e[0] < 0:
        e = -e
    return F32(2) * e[1:], _R32(q1)                     # (float32 arrays: lock_rows' R_1 @ (2 e_v) is a float32 product)


def _position_f32(bodies, a):
    x1, a1, u, x2, a2 = sd.sides_given(bodies, a)      # (float32 R anchor, R axis: jd.side is _side_f32 here)
    err = ((x1 + a1) - (x2 + a2)).astype(F32)          # diff_of_sums: exact to an ulp of the error
    u = u.astype(F32)
    return float(u[0] * err[0] + u[1] * err[1] + u[2] * err[2])


@contextlib.contextmanager
def float32_rows(sides_only=False):
    """inside, the dense references assemble joint rows from float32 evaluations of what the device evaluates"""
    saved = jd.side, lm.angle_of, sd.lock_error, sd.position
    jd.side = _side_f32
    if not sides_only:
        lm.angle_of, sd.lock_error, sd.position = _angle_of_f32, _lock_error_f32, _position_f32
    try:
        yield
    finally:
        jd.side, lm.angle_of, sd.lock_error, sd.position = saved


def round_rows(I):
    """the island's J and c as float32 numbers (contact rows too: they are a float32 batch's as well), A and b from them"""
    if not I.m:
        return I
    r = lambda x: np.asarray(x, np.float64).astype(F32).astype(np.float64)
    I.J, I.c = r(I.J), r(I.c)
    I.A = I.J @ I.minv(I.J.T) + np.diag(I.cfm / I.h)
    I.b = I.c / I.h - I.J @ (I.v / I.h + I.minv(I.f))
    return I


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


def model_per_slot(result, joint_term=True):
    """M_v of every body slot over all islands of a Result (0 for slots in no island: dead ones)"""
    if not joint_term:
        out = np.zeros(result.bodies.n)
        for I, lam in zip(result.islands, result.lams):
            out[np.asarray(I.slots, int)] = body_model(I, lam, False)
        return out
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


def deviation(result, lvel, avel, joint_term=True):
    """per body slot, the largest |v - v_ref| of its six components in units of eps32 M_v(body)"""
    d = np.maximum(np.max(np.abs(np.asarray(lvel, np.float64) - result.bodies.lvel), axis=1),
                   np.max(np.abs(np.asarray(avel, np.float64) - result.bodies.avel), axis=1))
    mv = model_per_slot(result, joint_term)
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


OLD_RULE_ROWS = 700          # the largest island the old rule ever admitted had 604 rows; kappa of thousands of rows is minutes


def old_allowance(result, world, live):
    """the largest velocity error the rule before the band allowed over the live bodies -- 10 eps32 kappa(A) x max(|v_ref|, g h) --
    or None where that rule did not admit the tick: a tolerance above 1e-3, or a clamp margin below 1e-3 of the largest |lambda|"""
    if max([I.m for I in result.islands] + [0]) > OLD_RULE_ROWS:
        return None                                             # (kappa >= 3e3 on every such island of the suite: not admitted)
    t = 10 * EPS32 * max([I.kappa() for I in result.islands] + [1.0])
    if t > 1e-3 or not gate_passes(result):
        return None
    return t * ld.velocity_scale(result.bodies, world, live)


def assert_in_old_allowance(result, world, post, live, what="float32 QuickStep"):
    """The joint files' second assertion.  With the joint term the band is per body and needs no gate, but on a well-conditioned
    island it allows more than 10 eps32 kappa did -- (ERP / h) eps32 |a| is what the rows' inputs CAN carry, and kappa ~ 1 allowed
    less -- so wherever the old rule admits the tick its allowance holds as well: nothing that was asserted is asserted no more"""
    post = np.asarray(post, np.float64)
    a = old_allowance(result, world, live)
    if a is None:
        return None
    err = ld.velocity_error(result.bodies, post[:, 7:10], post[:, 10:13], live)
    assert err <= a, f"{what}: velocity error {err:.3e} above the old allowance {a:.3e}"
    xerr = np.max(np.abs(post[live, 0:3] - result.bodies.pos[live]))
    assert xerr <= a * world.h + 4 * EPS32 * max(1.0, np.max(np.abs(result.bodies.pos[live]))), f"{what}: position error {xerr:.3e}"
    qerr = np.max(np.abs(post[live, 3:7] - result.bodies.quat[live]))
    assert qerr <= a * world.h + 4 * EPS32, f"{what}: quaternion error {qerr:.3e}"
    return err / a


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


def as_f32_joint_inputs(B, W, jts, art, lim):
    """as_f32_inputs with the articulation joints and their limots (None stays None)"""
    r = lambda x: np.asarray(x, np.float64).astype(np.float32).astype(np.float64)
    B2, W2, j2 = as_f32_inputs(B, W, jts)
    a2 = art.copy()
    for f in ("anchor1", "anchor2", "axis1", "axis2"):
        a2[f] = r(art[f])
    l2 = None
    if lim is not None:
        l2 = lim.copy()
        for f in lm.LIMOT_DTYPE.names:
            l2[f] = r(lim[f])
    return B2, W2, j2, a2, l2


def joint_reference(B, W, jts, art, lim, stepper="quick"):
    """the reference's tick of a float32 batch holding these inputs, every island with its joint term attached
    -> (Result, the inputs as the batch holds them: Bodies, World, contact joints, joints, limots)"""
    B2, W2, j2, a2, l2 = as_f32_joint_inputs(B, W, jts, art, lim)
    r = sd.step(B2, W2, j2, a2, l2, stepper)
    return attach_joint_term(r, B2, W2, j2, a2, l2), (B2, W2, j2, a2, l2)


def joint_emulation(r, inputs, rows=True):
    """population (b) for islands with joint rows, against the reference r = joint_reference(...)[0] of the same inputs: the float32
    sweeps on the reference's own A and b (rows = False), or on rows a float32 batch would have made (float32_rows, round_rows)
    -> (lvel, avel) per slot; kinematic bodies and bodies in no island keep the reference's"""
    B2, W2, j2, a2, l2 = inputs
    if rows == "sides":                   # R anchor and R axis alone: the emulation JOINT_MEASURED["rows"] was measured with
        with float32_rows(sides_only=True):
            islands = sd.step(B2, W2, j2, a2, l2, "quick").islands
    elif rows:
        with float32_rows():
            islands = [round_rows(I) for I in sd.step(B2, W2, j2, a2, l2, "quick").islands]
    else:
        islands = r.islands
    lv, av = r.bodies.lvel.copy(), r.bodies.avel.copy()
    for I in islands:
        if not I.m:
            continue
        v = I.velocities(emulate_f32(I, W2.iters, W2.sor_w).astype(np.float64)).reshape(-1, 6)
        free = np.array([not (B2.flags[s] & ld.KINEMATIC) for s in I.slots])
        sl = np.asarray(I.slots, int)[free]
        lv[sl], av[sl] = v[free, :3], v[free, 3:]
    return lv, av
