"""A dense float64 restatement of one contact-joint tick (dWorldStep / dWorldQuickStep), written from the definitions.

Test infrastructure, not a test file.  It is a second route to the numbers the HIP island solvers (csrc/dmx_lcp.hip,
csrc/dmx_islands.hip) and the CPU oracle (oracle/orc_step.c) produce, built from

  * SURVEY.md section 8, row a-7 (island construction, body stage, rows, the two steppers, integration);
  * the system stated in include/dmx_batch.h at dmxBatchSetStepper:
        A lambda = b + w,  A = J M^-1 J^T + diag(cfm / h),  lo <= lambda <= hi,  w complementary to lambda;
  * ODE's contact-joint semantics (dxJointContact::getInfo1 / getInfo2): one row per contact with mu <= 0, three
    otherwise; the normal row's c = erp * max(depth, 0) / h raised by the bounce rule; friction directions from dPlaneSpace;
    dContactSoftERP / dContactSoftCFM replace the world's ERP / the normal row's CFM.

Everything is float64 on dense matrices: no accumulators, no sparsity, no row scaling.  QuickStep is projected SOR on the
dense system (`quickstep`); dWorldStep is a mixed box LCP solved by block principal pivoting with Murty's single-flip
rule as the fallback (`exact`), whose answer is certified against the KKT conditions before it is returned.
"""
import numpy as np

ALIVE, KINEMATIC, NOGRAVITY, NOGYRO = 1, 2, 4, 8
CONTACT_BOUNCE, CONTACT_SOFT_ERP, CONTACT_SOFT_CFM = 0x004, 0x008, 0x010
GYRO_OFF, GYRO_EXPLICIT, GYRO_IMPLICIT = 0, 1, 2
FREE, AT_LO, AT_HI = 0, 1, 2

# the fields of dmxContactJoint (include/dmx_batch.h), in order; batch.CONTACT_JOINT_DTYPE is the C layout of the same
JOINT_FIELDS = [("pos", np.float64, (3,)), ("normal", np.float64, (3,)), ("depth", np.float64), ("body1", np.int32),
                ("body2", np.int32), ("mode", np.int32), ("mu", np.float64), ("bounce", np.float64),
                ("bounce_vel", np.float64), ("soft_erp", np.float64), ("soft_cfm", np.float64)]
JOINT_DTYPE = np.dtype(JOINT_FIELDS)


class ReferenceError(AssertionError):
    """The reference could not certify its own answer: a broken reference, never a pass."""


# ---------------------------------------------------------------------------------------------------------------------
# small geometry
def cross_matrix(a):
    """[a]x, the matrix with [a]x v = a x v"""
    return np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])


def quat_to_R(q):
    """rotation matrix of the unit quaternion q = (w, x, y, z)"""
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def quat_mul(a, b):
    """Hamilton product a (x) b, (w, x, y, z)"""
    aw, av = a[0], np.asarray(a[1:])
    bw, bv = b[0], np.asarray(b[1:])
    return np.concatenate([[aw * bw - av @ bv], aw * bv + bw * av + np.cross(av, bv)])


def plane_space(n):
    """dPlaneSpace: unit t1, t2 with (t1, t2, n) right-handed.  ODE picks the construction by the normal's largest
    component: with |n_z| > 1/sqrt(2), t1 is n projected out of the x axis' complement (t1 in the yz plane); otherwise
    t1 lies in the xy plane.  t2 = n x t1 completes the frame."""
    n = np.asarray(n, np.float64)
    if abs(n[2]) > np.sqrt(0.5):
        t1 = np.array([0.0, -n[2], n[1]])
    else:
        t1 = np.array([-n[1], n[0], 0.0])
    t1 /= np.linalg.norm(t1)
    t2 = np.cross(n, t1)
    return t1, t2


def joints(n, **fields):
    """a zeroed joint array of n entries (JOINT_DTYPE), fields set from keyword arguments"""
    j = np.zeros(n, JOINT_DTYPE)
    for k, v in fields.items():
        j[k] = v
    return j


# ---------------------------------------------------------------------------------------------------------------------
class World:
    """world parameters of one tick"""

    def __init__(self, h=1.0 / 60.0, gravity=(0.0, -9.8, 0.0), erp=0.2, cfm=1e-10, iters=20, sor_w=1.3, gyro=GYRO_OFF):
        self.h, self.gravity, self.erp, self.cfm = float(h), np.asarray(gravity, np.float64), float(erp), float(cfm)
        self.iters, self.sor_w, self.gyro = int(iters), float(sor_w), int(gyro)


class Bodies:
    """per-body state: pos (n,3), quat (n,4) wxyz, lvel, avel (n,3), mass (n,), inertia (n,3) body-frame principal, flags"""

    def __init__(self, pos, quat, lvel, avel, mass, inertia, flags=None):
        f = lambda a, k: np.array(a, np.float64).reshape(-1, k)
        self.pos, self.quat, self.lvel, self.avel = f(pos, 3), f(quat, 4), f(lvel, 3), f(avel, 3)
        self.mass, self.inertia = np.array(mass, np.float64).reshape(-1), f(inertia, 3)
        self.n = len(self.pos)
        self.flags = np.full(self.n, ALIVE, np.uint8) if flags is None else np.asarray(flags, np.uint8).copy()

    def copy(self):
        return Bodies(self.pos, self.quat, self.lvel, self.avel, self.mass, self.inertia, self.flags)


# ---------------------------------------------------------------------------------------------------------------------
def canonical(bodies, jts):
    """the header's contract: a slot that is -1, out of range or not alive is static; a static body1 with a live body2
    swaps the two and reverses the normal; static-static joints and self-joints are dropped.
    -> list of (joint index, b1, b2 or -1, normal pointing into b1)"""
    live = lambda s: 0 <= s < bodies.n and bool(bodies.flags[s] & ALIVE)
    out = []
    for k, j in enumerate(jts):
        b1 = int(j["body1"]) if live(int(j["body1"])) else -1
        b2 = int(j["body2"]) if live(int(j["body2"])) else -1
        nrm = np.array(j["normal"], np.float64)
        if b1 < 0 and b2 >= 0:
            b1, b2, nrm = b2, -1, -nrm
        if b1 < 0 or b1 == b2:
            continue
        out.append((k, b1, b2, nrm))
    return out


def islands(bodies, cj):
    """union-find over joints between two live bodies; -> list of (body slots ascending, canonical joints in creation order),
    islands ordered by their lowest slot; every live body is in exactly one island"""
    parent = list(range(bodies.n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for _, b1, b2, _ in cj:
        if b2 >= 0:
            r1, r2 = find(b1), find(b2)
            if r1 != r2:
                parent[max(r1, r2)] = min(r1, r2)
    live = [s for s in range(bodies.n) if bodies.flags[s] & ALIVE]
    groups = {}
    for s in live:
        groups.setdefault(find(s), []).append(s)
    by_root = {}
    for c in cj:
        by_root.setdefault(find(c[1]), []).append(c)
    return [(groups[root], by_root.get(root, [])) for root in sorted(groups)]


def body_stage(bodies, world, s):
    """-> (inverse mass, world inverse inertia 3x3, force, torque) of slot s: gravity, invI_w = R diag(1/I) R^T, gyroscopic
    torque; a kinematic body has zero inverse mass and inertia and no applied force"""
    fl = int(bodies.flags[s])
    if fl & KINEMATIC:
        return 0.0, np.zeros((3, 3)), np.zeros(3), np.zeros(3)
    m, Ib = bodies.mass[s], bodies.inertia[s]
    R = quat_to_R(bodies.quat[s])
    invI = R @ np.diag(1.0 / Ib) @ R.T
    f = np.zeros(3) if fl & NOGRAVITY else m * world.gravity
    tau = np.zeros(3)
    isotropic = Ib[0] == Ib[1] == Ib[2]          # w x (I w) = I (w x w) = 0 exactly: no gyroscopic torque
    if world.gyro != GYRO_OFF and not (fl & NOGYRO) and not isotropic:
        Iw = R @ np.diag(Ib) @ R.T
        w = bodies.avel[s]
        L = Iw @ w
        if world.gyro == GYRO_EXPLICIT:
            tau = -np.cross(w, L)
        else:
            # Lacoursiere's implicit form (SURVEY a-7): I~ = I_w - h [L]x,  tau = (I_w I~^-1 - 1) L / h
            It = Iw - world.h * cross_matrix(L)
            tau = (Iw @ np.linalg.inv(It) - np.eye(3)) @ L / world.h
    return 1.0 / m, invI, f, tau


class Island:
    """the dense system of one island"""

    def __init__(self, bodies, world, slots, cj, jts):
        self.h = h = world.h
        self.slots = list(slots)
        loc = {s: k for k, s in enumerate(self.slots)}
        nb = len(self.slots)
        self.Mblk = np.zeros((nb, 6, 6))             # M^-1, block diagonal: one 6 x 6 block per body
        self.f = np.zeros(6 * nb)
        self.v = np.zeros(6 * nb)
        for k, s in enumerate(self.slots):
            im, invI, f, tau = body_stage(bodies, world, s)
            self.Mblk[k, :3, :3] = im * np.eye(3)
            self.Mblk[k, 3:, 3:] = invI
            self.f[6 * k:6 * k + 6] = np.concatenate([f, tau])
            self.v[6 * k:6 * k + 6] = np.concatenate([bodies.lvel[s], bodies.avel[s]])
        rows_J, c, cfm, lo, hi, self.row_joint, self.row_kind = [], [], [], [], [], [], []
        for ji, b1, b2, n in cj:
            j = jts[ji]
            mode, mu = int(j["mode"]), max(float(j["mu"]), 0.0)
            p = np.asarray(j["pos"], np.float64)
            c1 = p - bodies.pos[b1]
            c2 = p - bodies.pos[b2] if b2 >= 0 else None
            dirs = [n] + (list(plane_space(n)) if mu > 0 else [])
            for kind, d in enumerate(dirs):
                J = np.zeros(6 * nb)
                J[6 * loc[b1]:6 * loc[b1] + 6] = np.concatenate([d, np.cross(c1, d)])
                if b2 >= 0:
                    J[6 * loc[b2]:6 * loc[b2] + 6] = np.concatenate([-d, -np.cross(c2, d)])
                rows_J.append(J)
                self.row_joint.append(ji)
                self.row_kind.append(kind)
                if kind == 0:
                    erp = float(j["soft_erp"]) if mode & CONTACT_SOFT_ERP else world.erp
                    cval = erp * max(float(j["depth"]), 0.0) / h
                    if mode & CONTACT_BOUNCE:
                        outgoing = J @ self.v
                        if j["bounce_vel"] >= 0 and -outgoing > j["bounce_vel"]:
                            cval = max(cval, -float(j["bounce"]) * outgoing)
                    c.append(cval)
                    cfm.append(float(j["soft_cfm"]) if mode & CONTACT_SOFT_CFM else world.cfm)
                    lo.append(0.0)
                    hi.append(np.inf)
                else:
                    c.append(0.0)
                    cfm.append(world.cfm)
                    lo.append(-mu)
                    hi.append(mu)
        self.m = len(rows_J)
        self.J = np.array(rows_J).reshape(self.m, 6 * nb)
        self.c, self.cfm = np.array(c), np.array(cfm)
        self.lo, self.hi = np.array(lo), np.array(hi)
        self.row_joint, self.row_kind = np.array(self.row_joint, int), np.array(self.row_kind, int)
        self.A = self.J @ self.minv(self.J.T) + np.diag(self.cfm / h)
        self.b = self.c / h - self.J @ (self.v / h + self.minv(self.f))
        self.nu = int(np.sum(np.isinf(self.lo) & np.isinf(self.hi)))
        self.nbd = self.m - self.nu

    def kappa(self):
        """2-norm condition number of A (symmetric positive definite)"""
        if self.m == 0:
            return 1.0
        ev = np.linalg.eigvalsh(self.A)
        return float(ev[-1] / ev[0])

    # ---- QuickStep -------------------------------------------------------------------------------------------------
    def quickstep(self, iters, w, order=None):
        """projected SOR from lambda = 0, rows in creation order (or `order`) every sweep:
        lambda_i <- clamp(lambda_i + w (b_i - (A lambda)_i) / A_ii).  -> (lambda, margin): margin = the smallest distance
        by which an unclamped update missed a finite bound, or by which a clamped one overshot it"""
        lam = np.zeros(self.m)
        margin = np.inf
        A, b, lo, hi = self.A, self.b, self.lo, self.hi
        rows = range(self.m) if order is None else order
        for _ in range(iters):
            for i in rows:
                x = lam[i] + w * (b[i] - A[i] @ lam) / A[i, i]
                if np.isfinite(lo[i]):
                    margin = min(margin, abs(x - lo[i]))
                if np.isfinite(hi[i]):
                    margin = min(margin, abs(x - hi[i]))
                lam[i] = min(max(x, lo[i]), hi[i])
        return lam, margin

    # ---- dWorldStep ----------------------------------------------------------------------------------------------------
    def _solve_state(self, state):
        lam = np.where(state == AT_LO, self.lo, np.where(state == AT_HI, self.hi, 0.0))
        F = state == FREE
        if F.any():
            C = ~F
            rhs = self.b[F] - (self.A[np.ix_(F, C)] @ lam[C] if C.any() else 0.0)
            AF = self.A[np.ix_(F, F)]
            L = np.linalg.cholesky(AF)
            x = np.linalg.solve(L.T, np.linalg.solve(L, rhs))
            # two steps of iterative refinement (the certificate asks for |w| <= 1e-12 ||b|| on islands with kappa ~ 1e9)
            for _ in range(2):
                x = x + np.linalg.solve(L.T, np.linalg.solve(L, rhs - AF @ x))
            lam[F] = x
        return lam, self.A @ lam - self.b

    def _w(self, lam):
        """w = A lambda - b, summed in extended precision"""
        return np.asarray(self.A.astype(np.longdouble) @ lam.astype(np.longdouble) - self.b, np.float64)

    def _infeasible(self, state, lam, w, tol_w, tol_l):
        bad = np.zeros(self.m, bool)
        F = state == FREE
        bad |= F & ((lam < self.lo - tol_l) | (lam > self.hi + tol_l))
        bad |= (state == AT_LO) & (w < -tol_w)
        bad |= (state == AT_HI) & (w > tol_w)
        return bad

    def exact(self, max_rounds=None):
        """the mixed box LCP, solved by block principal pivoting (Judice-Pires: flip every infeasible row) with Murty's
        single flip of the last infeasible row once the count of infeasible rows stops falling -- finite for a positive
        definite A.  The answer is certified against the KKT conditions (relative to ||b||) before it is returned:
        |w| <= 1e-12 on free rows, lambda inside its bounds, w >= 0 at lo, w <= 0 at hi; ReferenceError otherwise.
        -> (lambda, info) with info = {rounds, n_lo, n_hi, murty}"""
        m = self.m
        if m == 0:
            return np.zeros(0), {"rounds": 0, "n_lo": 0, "n_hi": 0, "murty": 0}
        scale = max(np.linalg.norm(self.b), 1e-300)
        tol_w = 1e-13 * scale
        state = np.full(m, FREE)
        best, stall, murty = m + 1, 0, 0
        max_rounds = max_rounds or 50 * m + 100
        for rnd in range(max_rounds):
            lam, w = self._solve_state(state)
            tol_l = 1e-13 * max(1.0, np.max(np.abs(lam)))
            bad = self._infeasible(state, lam, w, tol_w, tol_l)
            nbad = int(bad.sum())
            if nbad == 0:
                break
            if nbad < best:
                best, stall = nbad, 0
            else:
                stall += 1
            flip = np.nonzero(bad)[0]
            if stall >= 3 or murty:             # once the block flips stall, single flips to the end (finite)
                flip = flip[-1:]
                murty += 1
            for i in flip:
                if state[i] == FREE:
                    state[i] = AT_LO if lam[i] < self.lo[i] else AT_HI
                else:
                    state[i] = FREE
        else:
            raise ReferenceError(f"exact(): no solution after {max_rounds} rounds (m = {m})")
        self.certify(lam, state)
        return lam, {"rounds": rnd + 1, "n_lo": int(np.sum(state == AT_LO)), "n_hi": int(np.sum(state == AT_HI)),
                     "murty": murty}

    def certify(self, lam, state):
        scale = max(np.linalg.norm(self.b), 1e-300)
        w = self._w(lam)
        tol = 1e-12 * scale
        tol_l = 1e-12 * max(1.0, np.max(np.abs(lam)))
        F = state == FREE
        errs = []
        if F.any() and np.max(np.abs(w[F])) > tol:
            errs.append(f"|w| on free rows {np.max(np.abs(w[F])):.3e} > {tol:.3e}")
        if np.any(lam < self.lo - tol_l) or np.any(lam > self.hi + tol_l):
            errs.append("lambda outside its bounds")
        if np.any(w[state == AT_LO] < -tol):
            errs.append(f"w < 0 at lo: {np.min(w[state == AT_LO]):.3e}")
        if np.any(w[state == AT_HI] > tol):
            errs.append(f"w > 0 at hi: {np.max(w[state == AT_HI]):.3e}")
        if errs:
            raise ReferenceError("exact(): KKT certificate failed: " + "; ".join(errs))

    def velocities(self, lam):
        """v' = v + h M^-1 (f + J^T lambda), per body 6 reals"""
        return self.v + self.h * self.minv(self.f + (self.J.T @ lam if self.m else 0.0))

    def minv(self, x):
        """M^-1 x for x of 6 nb rows (a vector or a matrix)"""
        nb = len(self.Mblk)
        xb = np.asarray(x, np.float64).reshape(nb, 6, -1)
        return np.einsum("kij,kjc->kic", self.Mblk, xb).reshape(np.shape(x))

    @property
    def Minv(self):
        """M^-1 as a dense matrix (small islands only)"""
        nb = len(self.Mblk)
        out = np.zeros((6 * nb, 6 * nb))
        for k in range(nb):
            out[6 * k:6 * k + 6, 6 * k:6 * k + 6] = self.Mblk[k]
        return out


class Result:
    """the tick's outcome: new state (Bodies), per island diagnostics, and lambda per canonical joint row"""

    def __init__(self, bodies, isl, lams, infos, margins):
        self.bodies, self.islands, self.lams, self.infos, self.margins = bodies, isl, lams, infos, margins

    def normal_lambda(self, n_joints):
        """the normal row's lambda of every input joint (NaN for joints the stepper dropped)"""
        out = np.full(n_joints, np.nan)
        for I, lam in zip(self.islands, self.lams):
            k = I.row_kind == 0
            out[I.row_joint[k]] = lam[k]
        return out


def step(bodies, world, jts, stepper="quick", order=None):
    """one tick: islands, rows, solve (stepper "quick" = QuickStep's SOR, "exact" = dWorldStep), integration.
    -> Result.  `bodies` is not changed."""
    jts = np.asarray(jts, JOINT_DTYPE) if len(jts) else np.zeros(0, JOINT_DTYPE)
    cj = canonical(bodies, jts)
    out = bodies.copy()
    isl, lams, infos, margins = [], [], [], []
    h = world.h
    for slots, cjs in islands(bodies, cj):
        I = Island(bodies, world, slots, cjs, jts)
        if stepper == "quick":
            lam, margin = I.quickstep(world.iters, world.sor_w, order)
            info = {}
        else:
            lam, info = I.exact()
            margin = None
        v = I.velocities(lam)
        for k, s in enumerate(slots):
            if bodies.flags[s] & KINEMATIC:
                lv, av = bodies.lvel[s], bodies.avel[s]
            else:
                lv, av = v[6 * k:6 * k + 3], v[6 * k + 3:6 * k + 6]
            out.lvel[s], out.avel[s] = lv, av
            out.pos[s] = bodies.pos[s] + h * lv
            q = bodies.quat[s] + 0.5 * h * quat_mul(np.concatenate([[0.0], av]), bodies.quat[s])
            out.quat[s] = q / np.linalg.norm(q)
        isl.append(I)
        lams.append(lam)
        infos.append(info)
        margins.append(margin)
    return Result(out, isl, lams, infos, margins)


def velocity_error(ref, lvel, avel, slots=None):
    """largest |v - v_ref| over linear and angular velocities (absolute: callers scale it with velocity_scale)"""
    sl = slice(None) if slots is None else slots
    d = max(np.max(np.abs(np.asarray(lvel, np.float64)[sl] - ref.lvel[sl]), initial=0.0),
            np.max(np.abs(np.asarray(avel, np.float64)[sl] - ref.avel[sl]), initial=0.0))
    return d


def velocity_scale(ref, world, slots=None):
    """max(|v_ref|, g h) over linear and angular velocities (g = |gravity|): what tolerances are relative to"""
    sl = slice(None) if slots is None else slots
    return max(np.max(np.abs(ref.lvel[sl]), initial=0.0), np.max(np.abs(ref.avel[sl]), initial=0.0),
               np.linalg.norm(world.gravity) * world.h)
