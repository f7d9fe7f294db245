"""Friction that scales with the normal force (dContactApprox1), as a dense float64 restatement on top of lcp_dense.

Test infrastructure, not a test file.  The definitions are those of include/dmx_batch.h at DMX_CONTACT_APPROX1:

  * friction row d (1 or 2) of a contact joint is a PYRAMID ROW when bit DMX_CONTACT_APPROX1_d of its mode is set and
    0 < mu < inf; every other row is what lcp_dense.Island makes of it (mu = inf: unbounded, mu <= 0: no friction rows);
  * QuickStep: when a pyramid row is visited in a sweep its bounds are -/+ |mu lambda_n|, lambda_n = the current multiplier
    of the contact's normal row (rows in creation order, so already updated in this sweep);
  * dWorldStep: pass A solves the box LCP with every pyramid row held at lo = hi = 0, pass B solves it with the pyramid
    rows bounded by -/+ mu lambda^A_n; pass B's lambda is the tick's.
"""
import numpy as np

import lcp_dense as D

APPROX1_1, APPROX1_2, APPROX1 = 0x1000, 0x2000, 0x3000
APPROX1_N = 0x4000          # ODE's rolling-friction bit: without meaning here


class Island(D.Island):
    """lcp_dense.Island with the pyramid rows marked: pyr_mu[i] > 0 on a pyramid row (0 elsewhere), pyr_n[i] = its normal row"""

    def __init__(self, bodies, world, slots, cj, jts):
        super().__init__(bodies, world, slots, cj, jts)
        self.pyr_mu = np.zeros(self.m)
        self.pyr_n = np.full(self.m, -1, int)
        for i in range(self.m):
            kind = int(self.row_kind[i])
            if kind == 0:
                continue
            j = jts[self.row_joint[i]]
            mu = max(float(j["mu"]), 0.0)
            if (int(j["mode"]) & (APPROX1_1 << (kind - 1))) and 0.0 < mu < np.inf:
                self.pyr_mu[i] = mu
                self.pyr_n[i] = i - kind          # rows of a contact: normal, direction 1, direction 2
        self.pyramid = self.pyr_mu > 0
        self.box_lo, self.box_hi = self.lo.copy(), self.hi.copy()

    def quickstep_pyramid(self, iters, w):
        """projected SOR as lcp_dense's quickstep, rows in creation order, with the moving bound of the pyramid rows.
        -> (lambda, margin); the margin counts the distance to the bound as it stood when the row was visited"""
        lam = np.zeros(self.m)
        margin = np.inf
        A, b = self.A, self.b
        for _ in range(iters):
            for i in range(self.m):
                lo, hi = self.box_lo[i], self.box_hi[i]
                if self.pyramid[i]:
                    hi = abs(self.pyr_mu[i] * lam[self.pyr_n[i]])
                    lo = -hi
                x = lam[i] + w * (b[i] - A[i] @ lam) / A[i, i]
                if np.isfinite(lo):
                    margin = min(margin, abs(x - lo))
                if np.isfinite(hi):
                    margin = min(margin, abs(x - hi))
                lam[i] = min(max(x, lo), hi)
        return lam, margin

    def _exact_margin(self, lam):
        """how far the certified solution is from changing its active set: free rows' distance to a finite bound, clamped
        rows' |w|"""
        w = self._w(lam)
        margin = np.inf
        for i in range(self.m):
            at_lo = np.isfinite(self.lo[i]) and lam[i] <= self.lo[i]
            at_hi = np.isfinite(self.hi[i]) and lam[i] >= self.hi[i]
            if at_lo or at_hi:
                if self.lo[i] < self.hi[i]:
                    margin = min(margin, abs(w[i]))
            else:
                if np.isfinite(self.lo[i]):
                    margin = min(margin, lam[i] - self.lo[i])
                if np.isfinite(self.hi[i]):
                    margin = min(margin, self.hi[i] - lam[i])
        return margin

    def exact_pyramid(self):
        """two calls of the certified exact(): pass A with the pyramid rows at lo = hi = 0, pass B with them bounded by
        -/+ mu lambda^A_n.  An island without pyramid rows: one call.  -> (lambda, info); info["margin"] = the smaller of the
        two passes' margins (pass B's counts the distance to the bounds pass A gave), info["lambda_a"] = pass A's lambda"""
        self.lo, self.hi = self.box_lo.copy(), self.box_hi.copy()
        if not self.pyramid.any():
            lam, info = self.exact()
            info["margin"] = self._exact_margin(lam)
            return lam, info
        p = self.pyramid
        self.lo[p] = 0.0
        self.hi[p] = 0.0
        lam_a, info_a = self.exact()
        margin_a = self._exact_margin(lam_a)
        bound = np.abs(self.pyr_mu[p] * lam_a[self.pyr_n[p]])
        self.lo[p], self.hi[p] = -bound, bound
        lam, info = self.exact()
        info["rounds"] += info_a["rounds"]
        info["murty"] += info_a["murty"]
        info["margin"] = min(margin_a, self._exact_margin(lam))
        info["lambda_a"] = lam_a
        return lam, info


def step(bodies, world, jts, stepper="quick"):
    """one tick as lcp_dense.step, with pyramid rows honoured.  -> lcp_dense.Result (margins: both steppers')"""
    jts = np.asarray(jts, D.JOINT_DTYPE) if len(jts) else np.zeros(0, D.JOINT_DTYPE)
    cj = D.canonical(bodies, jts)
    out = bodies.copy()
    isl, lams, infos, margins = [], [], [], []
    h = world.h
    for slots, cjs in D.islands(bodies, cj):
        I = Island(bodies, world, slots, cjs, jts)
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


def slope_scene(mass, theta, mu, mode, g=9.8, h=1.0 / 60.0, phi=0.0, cfm=0.0):
    """one box of mass `mass` with a huge inertia at rest, one contact with the plane y = 0 under it, gravity tilted by theta
    against the normal, downhill = (cos phi, 0, sin phi): -> (bodies, world, joints).  dPlaneSpace of the normal (0, 1, 0) gives
    t1 = (-1, 0, 0), t2 = (0, 0, 1).  (cfm = 0: A is the body's own 3 x 3 inverse mass, positive definite.)"""
    bodies = D.Bodies([[0.0, 0.5, 0.0]], [[1.0, 0.0, 0.0, 0.0]], [[0.0, 0.0, 0.0]], [[0.0, 0.0, 0.0]], [mass], [[1e12, 1e12, 1e12]])
    world = D.World(h=h, gravity=(g * np.sin(theta) * np.cos(phi), -g * np.cos(theta), g * np.sin(theta) * np.sin(phi)), cfm=cfm)
    jts = D.joints(1, pos=(0.0, 0.0, 0.0), normal=(0.0, 1.0, 0.0), depth=0.0, body1=0, body2=-1, mode=mode, mu=mu)
    return bodies, world, jts
