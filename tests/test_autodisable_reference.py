"""tests/autodisable_reference.py held to closed forms, and the scenes of tests/test_gpu_autodisable.py run through it alone
with the margin conditions asserted on every tick (autodisable_scenes.run_reference does).  CPU only."""
import math

import numpy as np
import pytest

import autodisable_reference as ar
import autodisable_scenes as sc
import lcp_dense as ld

H = sc.H
A, K, AD, DIS = sc.A, sc.K, sc.AD, sc.DIS


def run(B, W, params, ticks, joints=lambda t: [], stepper="quick", links=()):
    cnt = ar.Counters(B.n, params)
    out = []
    for t in range(ticks):
        tk = ar.step(B, W, joints(t), stepper, params, cnt, links)
        B, cnt = tk.bodies, tk.counters
        out.append(tk)
    return out


def first_asleep(ticks, s):
    """1-based tick at whose end slot s went to sleep, or None"""
    for t, tk in enumerate(ticks):
        if tk.bodies.flags[s] & DIS:
            return t + 1
    return None


def test_the_reference_and_the_contract_name_the_same_bits_and_defaults():
    """include/dmx_batch.h is the contract: its two bits, and ODE's defaults in its text, are the reference's and the package's"""
    import os
    import re
    from __graft_entry__ import ROOT, load_package
    src = open(os.path.join(ROOT, "include", "dmx_batch.h")).read()
    assert int(re.search(r"DMX_BODY_AUTODISABLE = (\d+)", src).group(1)) == ar.AUTODISABLE == load_package().batch.BODY_AUTODISABLE
    assert int(re.search(r"DMX_BODY_DISABLED = (\d+)", src).group(1)) == ar.DISABLED == load_package().batch.BODY_DISABLED
    assert "0.01, 0.01, 10, 0" in src
    p = ar.Params()
    assert (p.lin, p.ang, p.idle_steps, p.idle_time) == (0.01, 0.01, 10, 0.0)


@pytest.mark.parametrize("which", ["linear", "angular"])
@pytest.mark.parametrize("idle_steps,idle_time", [(10, 0.0), (0, 6.5 * H), (3, 6.5 * H), (9, 2.5 * H), (0, 0.0)])
def test_force_free_body_sleeps_after_exactly_the_idle_ticks_or_never(which, idle_steps, idle_time):
    p = ar.Params(lin=0.02, ang=0.03, idle_steps=idle_steps, idle_time=idle_time)
    W = sc.world(gravity=(0, 0, 0))
    want = max(idle_steps, math.ceil(idle_time / H), 1)          # (both zero: at the end of the first tick)
    for factor, expect in ((0.5, want), (2.0, None)):
        v = np.zeros((1, 3)); v[0, 1] = factor * (p.lin if which == "linear" else p.ang)
        B = sc.bodies([[0.0, 0.0, 0.0]], v if which == "linear" else None, v if which == "angular" else None, [A | AD])
        ticks = run(B, W, p, want + 5)
        if idle_steps == 0 and idle_time == 0.0:
            expect = 1           # the definition as written: the counters are reset to (0, 0), which is "run out"
        assert first_asleep(ticks, 0) == expect
        last = ticks[-1]
        if expect:
            assert np.all(last.bodies.lvel[0] == 0) and np.all(last.bodies.avel[0] == 0)
            # frozen from the tick it fell asleep: the pose of that tick's end
            assert np.array_equal(last.bodies.pos, ticks[expect - 1].bodies.pos) and last.skipped_islands == 1
        else:
            assert last.counters.steps[0] == idle_steps and last.counters.time[0] == idle_time


def test_bodies_the_rule_does_not_look_at():
    p = ar.Params(idle_steps=1)
    W = sc.world(gravity=(0, 0, 0))
    B = sc.bodies(np.zeros((4, 3)), flags=[A | AD | K, A, 0, AD])          # kinematic, without the bit, dead, dead with the bit
    ticks = run(B, W, p, 3)
    assert np.array_equal(ticks[-1].bodies.flags, B.flags)
    assert np.all(ticks[-1].counters.steps == 1)


@pytest.mark.parametrize("idle_steps", [3, 10])
def test_apex_window(idle_steps):
    s = sc.apex(idle_steps)
    g, thr, v0 = 9.8, s.params.lin, 0.9
    window = [k for k in range(1, s.ticks + 1) if abs(v0 - k * g * H) <= thr]
    assert len(window) == 6 and abs(2 * thr / (g * H) - len(window)) < 1        # 6.1 ticks
    ticks = sc.run_reference(s, "quick")
    if idle_steps < len(window):
        t = first_asleep(ticks, 0)
        assert t == window[0] + idle_steps - 1
        assert ticks[t - 1].bodies.pos[0, 1] > 5.0              # in mid-air, above where it started
        assert np.array_equal(ticks[-1].bodies.pos, ticks[t - 1].bodies.pos)
    else:
        assert first_asleep(ticks, 0) is None
        left = [tk.counters.steps[0] for tk in ticks]
        assert left[window[-1] - 1] == idle_steps - len(window) and left[window[-1]] == idle_steps      # reset on leaving


def test_island_rule_on_hand_made_graphs():
    # 0 awake - 1 - 2 - 3 asleep (a chain of contact joints); 4 - 5 asleep; 6 asleep alone; 7 awake alone
    n = 8
    flags = np.full(n, A | AD | DIS, np.uint8); flags[0] = A | AD; flags[7] = A | AD
    B = sc.bodies(np.column_stack([np.arange(n) * 2.0, np.zeros(n), np.zeros(n)]), flags=flags)
    pairs = [(1, 0), (2, 1), (3, 2), (5, 4)]
    j = ld.joints(len(pairs), body1=[a for a, _ in pairs], body2=[b for _, b in pairs], normal=(1.0, 0.0, 0.0), depth=0.0,
                  pos=[(2.0 * a - 1.0, 0.0, 0.0) for a, _ in pairs])
    p = ar.Params(idle_steps=100)
    tk = ar.step(B, sc.world(gravity=(0, 0, 0)), j, "quick", p, ar.Counters(n, p, steps=np.arange(n) + 2))
    assert tk.woken == [1, 2, 3] and tk.skipped_islands == 2 and tk.asleep_before == [4, 5, 6]
    assert tk.stepped == [0, 1, 2, 3, 7] and tk.contacts == 3
    assert not np.any(tk.bodies.flags[[0, 1, 2, 3, 7]] & DIS) and np.all(tk.bodies.flags[[4, 5, 6]] & DIS)
    # counters of woken bodies are not reset (they count down once, idle as they are); the asleep ones' keep their values
    assert list(tk.counters.steps) == [1, 2, 3, 4, 6, 7, 8, 8]
    # an articulation link is an island edge like a contact joint
    aw, asl = ar.split_islands(B, j[:0], links=((6, 7), (4, 5)))
    assert sorted(s for sl, _ in aw for s in sl) == [0, 6, 7] and [sl for sl, _ in asl] == [[1], [2], [3], [4, 5]]


@pytest.mark.parametrize("stepper", ["quick", "exact"])
@pytest.mark.parametrize("name", sorted(sc.SCENES))
def test_scenes_keep_the_margin_conditions(name, stepper):
    scene = sc.SCENES[name](stepper)
    ticks = sc.run_reference(scene, stepper)          # (asserts the conditions tick by tick)
    flags = ticks[-1].bodies.flags
    if name.startswith("free-"):
        n = scene.B.n
        for s in range(n):
            slow = s % 4 in (0, 3) and s not in ((4, 5, 6) if n >= 8 else ())
            assert first_asleep(ticks, s) == (5 if slow else None), s
    if name.startswith("settling"):
        heights = (1, 3, 6) if stepper == "exact" and name == "settling" else (1, 3)
        first = 0
        for hgt in heights:
            sl = list(range(first, first + hgt)); first += hgt
            if stepper == "quick" and hgt > 1 and name == "settling":
                assert not np.any(flags[sl] & DIS)               # the three-stack under QuickStep never rests
                continue
            # every member under its thresholds from the first tick on, so all asleep at the same tick: the tenth
            assert all(np.all(np.linalg.norm(tk.pre_lvel[sl], axis=1) < scene.params.lin) and
                       np.all(np.linalg.norm(tk.pre_avel[sl], axis=1) < scene.params.ang) for tk in ticks[:10])
            assert [first_asleep(ticks, s) for s in sl] == [10] * hgt
            assert np.all(ticks[-1].bodies.lvel[sl] == 0) and np.all(ticks[-1].bodies.avel[sl] == 0)
    if name == "waking":
        assert [tk.skipped_islands for tk in ticks] == [1, 1, 3, 2, 2]
        assert ticks[2].woken == [] and ticks[2].stepped == [3] and ticks[2].contacts == 0
        assert ticks[3].woken == [0, 1, 2] and ticks[3].contacts == 16
        assert not np.any(flags[[0, 1, 2, 3]] & DIS) and np.all(flags[[4, 5, 6]] & DIS)
        if stepper == "exact":       # the stack was idle while it rested: its counters went down, and waking did not put them back
            assert list(ticks[2].counters.steps[:3]) == [48, 48, 48] and list(ticks[3].counters.steps[:3]) == [47, 47, 47]
