"""The feedback of a tick -- the force and torque every joint and contact joint applied, include/dmx_batch.h at dmxBatchSetFeedback --
from the dense float64 restatement's own numbers (tests/slider_dense.py's Result: per island the Jacobian J, the multipliers
lambda and the bodies' slots).

Test infrastructure, not a test file; it shares no code with the device.  A constraint with rows r has J_r^T lambda_r summed over
its rows as its feedback: the 6-block of body 1 is (f1, t1), that of body 2 (f2, t2), a world side has none and reports zeros, and
an exchange of sides made for the canonical form is undone.  Which rows are whose: an island's articulation rows come first and
carry row_joint = -1, so they are mapped by the documented order -- the island's joints in canonical_arts order, per joint ball 3,
hinge 5, slider 5, fixed 6 rows, one more for a present limot -- and the contact rows behind them by row_joint."""
import numpy as np

import joint_dense as jd
import lcp_dense as ld
import limot_dense as lm
import slider_dense as sd

ROWS = {sd.BALL: 3, sd.HINGE: 5, sd.SLIDER: 5, sd.FIXED: 6}


def joint_rows(kind, limot):
    """rows of a joint of this kind; limot: its limot entry (None: none are set)"""
    has = kind in (sd.HINGE, sd.SLIDER) and limot is not None and lm.present(limot)
    return ROWS[int(kind)] + (1 if has else 0)


class Feedback:
    """joints [len(art), 4, 3], contacts [len(jts), 4, 3]: f1, t1, f2, t2 in the sides as given; *_island: the index of the
    island (in Result.islands) the joint or contact is in, -1 for the inactive and the dropped, which report zeros"""

    def __init__(self, na, nc):
        self.joints, self.contacts = np.zeros((na, 4, 3)), np.zeros((nc, 4, 3))
        self.joint_island, self.contact_island = np.full(na, -1), np.full(nc, -1)


def _blocks(I, lam, rows, loc, b1, b2, swapped):
    w = lam[rows] @ I.J[rows]                          # sum of lambda_r J_r: 6 reals per body of the island
    one = w[6 * loc[b1]:6 * loc[b1] + 6]
    two = w[6 * loc[b2]:6 * loc[b2] + 6] if b2 >= 0 else np.zeros(6)
    if swapped:
        one, two = two, one
    return np.array([one[:3], one[3:], two[:3], two[3:]])


def feedback(bodies, result, jts, art=None, lim=None):
    """-> Feedback of the tick `result` (slider_dense.step's or lcp_dense.step's) that started from `bodies`"""
    art = np.zeros(0, jd.ART_DTYPE) if art is None else art
    jts = np.asarray(jts, ld.JOINT_DTYPE) if len(jts) else np.zeros(0, ld.JOINT_DTYPE)
    out = Feedback(len(art), len(jts))
    members = jd.canonical_arts(bodies, art) + ld.canonical(bodies, jts)
    groups = ld.islands(bodies, members)
    assert len(groups) == len(result.islands)
    for n, ((slots, ms), I, lam) in enumerate(zip(groups, result.islands, result.lams)):
        assert list(slots) == list(I.slots)
        loc = {s: k for k, s in enumerate(I.slots)}
        r = 0
        for m in ms:
            if not isinstance(m[0], tuple):
                continue
            (_, k), b1, b2, swapped = m
            nr = joint_rows(art[k]["kind"], None if lim is None or len(lim) == 0 else lim[k])
            assert np.all(I.row_joint[r:r + nr] == -1)
            out.joints[k] = _blocks(I, lam, np.arange(r, r + nr), loc, b1, b2, swapped)
            out.joint_island[k] = n
            r += nr
        assert r == getattr(I, "n_art_rows", 0), "the articulation rows do not add up to the island's"
        for m in ms:
            if isinstance(m[0], tuple):
                continue
            k, b1, b2, _ = m
            rows = np.nonzero(I.row_joint == k)[0]
            assert len(rows) in (1, 3) and np.all(rows >= r)
            out.contacts[k] = _blocks(I, lam, rows, loc, b1, b2, int(jts[k]["body1"]) != b1)
            out.contact_island[k] = n
    return out


def net_wrench(bodies, b1, b2, fb, o=np.zeros(3)):
    """-> (f1 + f2, t1 + t2 + (x1 - o) x f1 + (x2 - o) x f2, the largest term) of a two-body constraint's feedback [4, 3]"""
    x1, x2 = bodies.pos[b1] - o, bodies.pos[b2] - o
    terms = [fb[1], fb[3], np.cross(x1, fb[0]), np.cross(x2, fb[2])]
    return fb[0] + fb[2], sum(terms), max(np.max(np.abs(t)) for t in terms + [fb[0], fb[2]])
