"""tests/stability_reference.py, the float64 restatement of a tick with damping, the angular speed cap and the contact correction
scalars, held to closed forms; and the scenes of tests/stability_scenes.py held to what their docstring promises.  CPU only."""
import numpy as np
import pytest

import autodisable_reference as ar
import lcp_dense as ld
import stability_reference as sr
import stability_scenes as sc

H = 1.0 / 60.0
IDENT = (1.0, 0.0, 0.0, 0.0)


def one_body(lvel=(0, 0, 0), avel=(0, 0, 0), flags=None, inertia=(1, 1, 1)):
    return ld.Bodies([(0.0, 1.0, 0.0)], [IDENT], [lvel], [avel], [2.0], [inertia], flags)


def world(**kw):
    kw.setdefault("gravity", (0, 0, 0))
    return ld.World(h=H, cfm=1e-5, **kw)


@pytest.mark.parametrize("stepper", ["quick", "exact"])
def test_free_body_decays_geometrically_down_to_the_threshold(stepper):
    s, thr = 0.1, 0.5
    B = one_body(lvel=(1.0, 0.0, 0.0), avel=(0.0, 2.0, 0.0))
    k = sr.Knobs(1).set_damping(s, s, thr, 2 * thr)
    v, w = [1.0], [2.0]
    for _ in range(12):
        B = sr.step(B, world(), [], stepper, k).bodies
        v.append(B.lvel[0, 0]); w.append(B.avel[0, 1])
    for seq, t in ((v, thr), (w, 2 * thr)):
        want = [seq[0]]
        for _ in range(12):
            want.append(want[-1] * (1 - s) if want[-1] * want[-1] > t * t else want[-1])
        assert np.allclose(seq, want, rtol=1e-15, atol=0)
        below = [x for x in seq if x * x <= t * t]
        assert len(below) >= 3 and len(set(below)) == 1          # constant from the first tick at or below the threshold
        assert np.allclose(seq[:len(seq) - len(below) + 1], seq[0] * (1 - s) ** np.arange(len(seq) - len(below) + 1), rtol=1e-14)


def test_the_comparison_with_the_threshold_is_strict_and_a_zero_scale_is_off():
    B = one_body(lvel=(0.5, 0.0, 0.0), avel=(0.0, 0.0, 0.25))
    k = sr.Knobs(1).set_damping(0.3, 0.3, 0.5, 0.25)                 # exactly on both thresholds
    r = sr.step(B, world(), [], "quick", k)
    assert np.array_equal(r.bodies.lvel, B.lvel) and np.array_equal(r.bodies.avel, B.avel)
    assert r.threshold_distance == [0.0, 0.0] and not sr.margin_ok(r)
    k = sr.Knobs(1).set_damping(0.0, 0.3, 0.1, 0.1)                  # linear scale zero: off, and no distance is reported for it
    r = sr.step(B, world(), [], "quick", k)
    assert np.array_equal(r.bodies.lvel, B.lvel) and np.allclose(r.bodies.avel[0, 2], 0.25 * 0.7, rtol=1e-15)
    assert len(r.threshold_distance) == 1 and sr.margin_ok(r)


def test_kinematic_bodies_are_neither_damped_nor_capped():
    B = one_body(lvel=(1.0, 0, 0), avel=(0, 3.0, 0), flags=[ld.ALIVE | ld.KINEMATIC])
    k = sr.Knobs(1).set_damping(0.5, 0.5, 0.0, 0.0).set_max_angular_speed(1.0)
    r = sr.step(B, world(), [], "quick", k)
    assert np.array_equal(r.bodies.lvel, B.lvel) and np.array_equal(r.bodies.avel, B.avel)
    assert np.allclose(r.bodies.pos[0], (H, 1.0, 0.0))


@pytest.mark.parametrize("spin", [0.5, 1.0, 4.0])
def test_spinning_isotropic_body_is_capped_and_its_quaternion_follows_the_capped_velocity(spin):
    mx = 1.0
    d = np.array([0.6, 0.0, 0.8])
    B = one_body(avel=spin * d)
    r = sr.step(B, world(), [], "quick", sr.Knobs(1).set_max_angular_speed(mx))
    av = r.bodies.avel[0]
    want = min(spin, mx)
    assert np.isclose(np.linalg.norm(av), want, rtol=1e-15) and np.allclose(av / np.linalg.norm(av), d, rtol=1e-15)
    if spin <= mx:
        assert np.array_equal(av, B.avel[0])          # (the test is strict: at the cap nothing is touched)
    q = np.array(IDENT) + 0.5 * H * ld.quat_mul(np.concatenate([[0.0], av]), np.array(IDENT))
    assert np.allclose(r.bodies.quat[0], q / np.linalg.norm(q), rtol=1e-15, atol=1e-17)


def centre_contact(depth, mode=0, bounce=0.0, bounce_vel=0.0):
    """one contact through the centre of mass along the normal, mu = 0"""
    return ld.joints(1, pos=(0.0, 1.0, 0.0), normal=(0.0, 1.0, 0.0), depth=depth, body1=0, body2=-1, mode=mode, mu=0.0, bounce=bounce,
                     bounce_vel=bounce_vel)


@pytest.mark.parametrize("stepper", ["quick", "exact"])
@pytest.mark.parametrize("depth,layer,vmax", [(0.03, 0.01, np.inf), (0.03, 0.01, 0.1), (0.03, 0.0, 0.1), (0.005, 0.01, 0.1), (0.01, 0.01, np.inf),
                                              (0.03, 0.0, np.inf)])
def test_push_out_velocity_of_a_resting_body(stepper, depth, layer, vmax):
    W = world()
    B = one_body()
    r = sr.step(B, W, centre_contact(depth), stepper, sr.Knobs(1, None, layer, vmax))
    vn = r.bodies.lvel[0, 1]
    want = min(W.erp * max(depth - layer, 0.0) / H, vmax)
    if depth <= layer:
        assert vn == 0.0                              # exactly
    else:
        # A lambda = c / h with A = 1 / m + cfm / h: v = h lambda / m = c / (1 + m cfm / h), the CFM term
        assert np.isclose(vn, want / (1.0 + 2.0 * W.cfm / H), rtol=1e-9 if stepper == "quick" else 1e-12)
    assert np.array_equal(r.bodies.lvel[0, [0, 2]], [0.0, 0.0]) and np.array_equal(r.bodies.avel[0], [0.0, 0.0, 0.0])


@pytest.mark.parametrize("stepper", ["quick", "exact"])
def test_a_bounce_above_the_clamp_survives(stepper):
    W = world()
    B = one_body(lvel=(0.0, -2.0, 0.0))
    jt = centre_contact(0.03, ld.CONTACT_BOUNCE, bounce=0.5, bounce_vel=0.1)
    r = sr.step(B, W, jt, stepper, sr.Knobs(1, None, 0.0, 0.1))
    assert r.islands[0].c[0] == 1.0 > 0.1                              # -bounce * outgoing, past the clamp
    assert np.isclose(r.bodies.lvel[0, 1], -2.0 + 3.0 / (1.0 + 2.0 * W.cfm / H), rtol=1e-9)      # v + (c - v) / (1 + m cfm / h)
    jt["bounce"] = 0.01                                                # a bounce below the clamped push-out: the clamp stands
    r = sr.step(B, W, jt, stepper, sr.Knobs(1, None, 0.0, 0.1))
    assert r.islands[0].c[0] == 0.1


@pytest.mark.parametrize("stepper", ["quick", "exact"])
@pytest.mark.parametrize("name", ["single-4", "stack-2", "exact-lds-30", "free"])
def test_defaults_reproduce_lcp_dense_bit_for_bit(name, stepper):
    s = sc.SCENES[name]()
    a = ld.step(s.B, s.W, s.jts, stepper)
    b = sr.step(s.B, s.W, s.jts, stepper, sr.Knobs(s.B.n))
    for f in ("pos", "quat", "lvel", "avel"):
        assert np.array_equal(getattr(a.bodies, f), getattr(b.bodies, f)), f
    for x, y in zip(a.lams, b.lams):
        assert np.array_equal(x, y)
    assert sr.Knobs(s.B.n).is_default() and not s.knobs.is_default()


SCENE_CASES = [(n, st) for n in sorted(sc.SCENES) for st in sc.SCENES[n]().steppers if n not in ("quick-1028", "quick-3076")]


@pytest.mark.parametrize("name,stepper", SCENE_CASES + [("quick-1028", "quick")])
def test_scenes_keep_the_margin_and_reach_both_sides_of_every_knob(name, stepper):
    """on the reference's own trajectory, in the values a float64 and a float32 batch hold.  (quick-3076 is built by the same
    function as quick-1028 and takes a dense 3 076-row system a tick: the GPU test asserts its margin on the ticks it compares.)"""
    s = sc.SCENES[name]()
    for prec in ("float64", "float32"):
        k = s.knobs.as_precision(prec)
        B = s.B
        for t in range(s.ticks):
            r = sr.step(B, s.W, s.jts, stepper, k, s.art)
            assert sr.margin_ok(r), (t, min(r.threshold_distance))
            if t == 0:
                first = r
            B = r.bodies
        r = first
        # the two extra slots keep their velocity bits
        for slot in (s.kinematic, s.slow):
            assert np.array_equal(r.bodies.lvel[slot], s.B.lvel[slot]) and np.array_equal(r.bodies.avel[slot], s.B.avel[slot])
        dyn = np.arange(s.B.n - 2)
        # damping: some body is scaled, some is not
        scaled = [i for i in dyn if not np.array_equal(r.damped.lvel[i], s.B.lvel[i]) or not np.array_equal(r.damped.avel[i], s.B.avel[i])]
        assert 0 < len(scaled) < len(dyn)
        # the cap: some spins end on it, some below it
        sp, mx = np.linalg.norm(r.bodies.avel[dyn], axis=1), k.table[dyn, sr.MAX_ANG_SPEED]
        on = np.isclose(sp, mx, rtol=1e-12)
        assert on.any() and (sp[~on] < mx[~on]).all() and (~on).any()
        if len(s.jts):
            d = s.jts["depth"]
            raw = s.W.erp * np.maximum(d - k.surface_layer, 0.0) / H
            assert (d < k.surface_layer).any() and (d > k.surface_layer).any()
            assert (raw > k.max_correcting_vel).any() and ((raw > 0) & (raw < k.max_correcting_vel)).any()
            c = np.concatenate([I.c[I.row_kind == 0] for I in r.islands if I.m])
            assert (c > k.max_correcting_vel).any(), "no bounce above the clamp"
            assert (c == k.max_correcting_vel).any() and (c == 0).any()


@pytest.mark.parametrize("stepper", ["quick", "exact"])
def test_the_sleepy_scene_keeps_both_margins_and_sleeps(stepper):
    """stability_scenes.sleepy_scene under stability_reference.step_autodisable: damping's margin and auto-disable's on every tick, the
    asleep islands bit for bit, and the three slow free bodies asleep by the end -- which they are not without damping"""
    s, p = sc.sleepy_scene()
    for knobs, want in ((s.knobs, 3), (sr.Knobs(s.B.n), 0)):
        B, cnt, slept = s.B, ar.Counters(s.B.n, p), []
        for t in range(s.ticks):
            tk = sr.step_autodisable(B, s.W, s.jts, stepper, knobs, p, cnt)
            assert sr.margin_ok(tk.result) and ar.margin_ok(tk, p, s.W.h), t
            for f in ("pos", "quat", "lvel", "avel"):
                assert np.array_equal(getattr(tk.bodies, f)[tk.asleep_before], getattr(B, f)[tk.asleep_before])
            assert len(tk.asleep_before) >= 4
            slept += tk.slept
            B, cnt = tk.bodies, tk.counters
        assert len(slept) == want, slept
