"""The rest of ODE's contact surface (mu2, fdir1, motion1 / 2 / N, slip1 / 2) as a dense float64 restatement on top of
friction_dense.Island: rows, bounds, c and a per-row cfm.

Test infrastructure, not a test file.  The definition is that of include/dmx_batch.h at DMX_CONTACT_MU2 (dmxBatchStepJointsSurface);
it shares no code with csrc/:

  * surfaces[k] belongs to joints[k]; bit X of the joint's mode says that field X of its surface is read;
  * mu_1 = max(mu, 0), mu_2 = max(mu2, 0) with MU2, else mu_1; three rows when max(mu_1, mu_2) > 0, else one;
  * row 0 along the canonical normal n; with FDIR1 d_1 = fdir1 as given and d_2 = n x d_1, else dPlaneSpace(n);
  * friction row r: mu_r = 0 gives lo = hi = 0, +inf the unbounded row, otherwise a pyramid row (APPROX1_r) or the box -/+ mu_r;
  * c of row 0 gains motionN before the bounce rule; c of row 1 / 2 is motion1 / motion2; the meaning is (v_p1 - v_p2) . d_r =
    c_r in canonical sides, d_2 = n x d_1: no motion changes sign where the sides were exchanged;
  * the cfm of row r is slip_r with SLIPr, else the world's.
"""
import numpy as np

import friction_dense as FD
import lcp_dense as D

MU2, FDIR1, MOTION1, MOTION2, MOTIONN, SLIP1, SLIP2 = 0x001, 0x002, 0x020, 0x040, 0x080, 0x100, 0x200
SURFACE_EXT = 0x3e3
APPROX1_1, APPROX1_2, APPROX1 = FD.APPROX1_1, FD.APPROX1_2, FD.APPROX1

# the fields of dmxContactSurface (include/dmx_batch.h), in order; batch.CONTACT_SURFACE_DTYPE is the C layout of the same
SURFACE_FIELDS = [("mu2", np.float64), ("fdir1", np.float64, (3,)), ("motion1", np.float64), ("motion2", np.float64),
                  ("motionN", np.float64), ("slip1", np.float64), ("slip2", np.float64)]
SURFACE_DTYPE = np.dtype(SURFACE_FIELDS)


def surfaces(n, **fields):
    """a zeroed surface array of n entries (SURFACE_DTYPE), fields set from keyword arguments"""
    s = np.zeros(n, SURFACE_DTYPE)
    for k, v in fields.items():
        s[k] = v
    return s


def coefficients(j, s):
    """-> (mu_1, mu_2) of joint j with surface s"""
    mu1 = max(float(j["mu"]), 0.0)
    mu2 = max(float(s["mu2"]), 0.0) if int(j["mode"]) & MU2 else mu1
    return mu1, mu2


class Island(FD.Island):
    """friction_dense.Island with every row rebuilt from the extended definition.  Beside the parent's fields: dirs (the row's
    direction), fmu / fdir (what the product keeps in RW_FMU / RW_FDIR: mu_r on a pyramid row, -1 on the normal row of a contact
    that has one, 0 elsewhere; the friction row's number)"""

    def __init__(self, bodies, world, slots, cj, jts, surfs):
        D.Island.__init__(self, bodies, world, slots, [], jts)          # the bodies' part: M^-1, f, v
        h = self.h
        loc = {s: k for k, s in enumerate(self.slots)}
        nb = len(self.slots)
        rows_J, c, cfm, lo, hi, rj, rk, dirs, pyr_mu = [], [], [], [], [], [], [], [], []
        for ji, b1, b2, n in cj:
            j, s = jts[ji], surfs[ji]
            mode = int(j["mode"])
            mus = (0.0,) + coefficients(j, s)
            p = np.asarray(j["pos"], np.float64)
            c1 = p - bodies.pos[b1]
            c2 = p - bodies.pos[b2] if b2 >= 0 else None
            ds = [n]
            if max(mus) > 0:
                if mode & FDIR1:
                    d1 = np.array(s["fdir1"], np.float64)
                    ds += [d1, np.cross(n, d1)]
                else:
                    ds += list(D.plane_space(n))
            motion = (float(s["motionN"]) if mode & MOTIONN else 0.0,
                      float(s["motion1"]) if mode & MOTION1 else 0.0,
                      float(s["motion2"]) if mode & MOTION2 else 0.0)
            slip = (None, float(s["slip1"]) if mode & SLIP1 else None, float(s["slip2"]) if mode & SLIP2 else None)
            for kind, d in enumerate(ds):
                J = np.zeros(6 * nb)
                J[6 * loc[b1]:6 * loc[b1] + 6] = np.concatenate([d, np.cross(c1, d)])
                if b2 >= 0:
                    J[6 * loc[b2]:6 * loc[b2] + 6] = np.concatenate([-d, -np.cross(c2, d)])
                rows_J.append(J)
                rj.append(ji)
                rk.append(kind)
                dirs.append(d)
                if kind == 0:
                    erp = float(j["soft_erp"]) if mode & D.CONTACT_SOFT_ERP else world.erp
                    cval = erp * max(float(j["depth"]), 0.0) / h + motion[0]
                    if mode & D.CONTACT_BOUNCE:
                        outgoing = J @ self.v
                        if j["bounce_vel"] >= 0 and -outgoing > j["bounce_vel"]:
                            cval = max(cval, -float(j["bounce"]) * outgoing)
                    c.append(cval)
                    cfm.append(float(j["soft_cfm"]) if mode & D.CONTACT_SOFT_CFM else world.cfm)
                    lo.append(0.0)
                    hi.append(np.inf)
                    pyr_mu.append(0.0)
                else:
                    mu = mus[kind]
                    pyramid = bool(mode & (APPROX1_1 << (kind - 1))) and 0.0 < mu < np.inf
                    c.append(motion[kind])
                    cfm.append(world.cfm if slip[kind] is None else slip[kind])
                    lo.append(-mu + 0.0)
                    hi.append(mu)
                    pyr_mu.append(mu if pyramid else 0.0)
        self.m = len(rows_J)
        self.J = np.array(rows_J).reshape(self.m, 6 * nb)
        self.dirs = np.array(dirs).reshape(self.m, 3)
        self.c, self.cfm = np.array(c), np.array(cfm)
        self.lo, self.hi = np.array(lo), np.array(hi)
        self.row_joint, self.row_kind = np.array(rj, int), np.array(rk, int)
        self.A = self.J @ self.minv(self.J.T) + np.diag(self.cfm / h)
        self.b = self.c / h - self.J @ (self.v / h + self.minv(self.f))
        self.nu = int(np.sum(np.isinf(self.lo) & np.isinf(self.hi)))
        self.nbd = self.m - self.nu
        self.pyr_mu = np.array(pyr_mu)
        self.pyr_n = np.where(self.pyr_mu > 0, np.arange(self.m) - self.row_kind, -1)
        self.pyramid = self.pyr_mu > 0
        self.box_lo, self.box_hi = self.lo.copy(), self.hi.copy()
        self.fmu = self.pyr_mu.copy()
        for i in np.nonzero(self.pyramid)[0]:
            self.fmu[self.pyr_n[i]] = -1.0
        self.fdir = self.row_kind.astype(np.float64)

    def quickstep_pyramid(self, iters, w):
        """the parent's sweeps; the margin leaves out the rows held at lo = hi (mu_r = 0): whatever the update proposes they end
        at that value, so no rounding can change what they do"""
        lam = np.zeros(self.m)
        margin = np.inf
        A, b = self.A, self.b
        for _ in range(iters):
            for i in range(self.m):
                lo, hi = self.box_lo[i], self.box_hi[i]
                held = lo == hi
                if self.pyramid[i]:
                    hi = abs(self.pyr_mu[i] * lam[self.pyr_n[i]])
                    lo = -hi
                x = lam[i] + w * (b[i] - A[i] @ lam) / A[i, i]
                if not held:
                    if np.isfinite(lo):
                        margin = min(margin, abs(x - lo))
                    if np.isfinite(hi):
                        margin = min(margin, abs(x - hi))
                lam[i] = min(max(x, lo), hi)
        return lam, margin


def step(bodies, world, jts, surfs, stepper="quick", drop_rows=None):
    """one tick as friction_dense.step with the extended surfaces honoured.  -> lcp_dense.Result (margins: both steppers').
    drop_rows(I) -> boolean mask of rows to delete from the island before it is solved (for the closed-form tests)"""
    jts = np.asarray(jts, D.JOINT_DTYPE) if len(jts) else np.zeros(0, D.JOINT_DTYPE)
    surfs = np.asarray(surfs, SURFACE_DTYPE) if len(surfs) else np.zeros(0, SURFACE_DTYPE)
    assert len(jts) == len(surfs)
    cj = D.canonical(bodies, jts)
    out = bodies.copy()
    isl, lams, infos, margins = [], [], [], []
    h = world.h
    for slots, cjs in D.islands(bodies, cj):
        I = Island(bodies, world, slots, cjs, jts, surfs)
        if drop_rows is not None:
            keep = ~drop_rows(I)
            assert not I.pyramid.any()
            for name in ("J", "c", "cfm", "lo", "hi", "row_joint", "row_kind", "b", "pyr_mu", "pyr_n", "pyramid", "box_lo", "box_hi"):
                setattr(I, name, getattr(I, name)[keep])
            I.A = I.A[np.ix_(keep, keep)]
            I.m = int(keep.sum())
        if stepper == "quick":
            lam, margin = I.quickstep_pyramid(world.iters, world.sor_w)
            info = {}
        else:
            lam, info = I.exact_pyramid()
            margin = info["margin"]
        v = I.velocities(lam)
        for k, s in enumerate(slots):
            if bodies.flags[s] & D.KINEMATIC:
                lv, av = bodies.lvel[s], bodies.avel[s]
            else:
                lv, av = v[6 * k:6 * k + 3], v[6 * k + 3:6 * k + 6]
            out.lvel[s], out.avel[s] = lv, av
            out.pos[s] = bodies.pos[s] + h * lv
            q = bodies.quat[s] + 0.5 * h * D.quat_mul(np.concatenate([[0.0], av]), bodies.quat[s])
            out.quat[s] = q / np.linalg.norm(q)
        isl.append(I)
        lams.append(lam)
        infos.append(info)
        margins.append(margin)
    return D.Result(out, isl, lams, infos, margins)
