"""dmxBatchRayCast on the device against tests/ray_reference.py, the float64 restatement of its definitions, by the band rule
stated there (K_RAY, K_N and C_GRAZE are that module's; tests/test_ray_reference.py measures them and checks, with the reference
alone, that every scene below leaves at most 0.2 % of its rays in the band, 5 % for the scene moved 8 km out).

Inputs are uploaded, then POS, QUAT and SIDES are downloaded again and THOSE feed the reference: what the device holds.  The
three forms -- a lane per ray, a wavefront per ray, brute force -- must agree bit for bit (ids and all seven reals): the winner
rule (smallest t, then plane < static boxes in order < bodies by slot) leaves nothing to the search order.  A form is forced
with set_ray_form; which kernel ran has no counter in the C ABI, the choice is by the setter (or the ray count) alone.
"""
import ctypes as C

import numpy as np
import pytest

from __graft_entry__ import load_package

import bp_scenes as sc
import ray_reference as rr
import ray_scenes as rs

pkg = load_package()
B = pkg.batch
pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32"]
H = 1.0 / 60.0
LANE, WAVE, BRUTE = B.RAY_FORM_LANE, B.RAY_FORM_WAVE, B.RAY_FORM_BRUTE


def _world(case, dtype, plane=rs.PLANE, gravity=(0.0, 0.0, 0.0), faces=True):
    w = pkg.BatchWorld(case.n, dtype=dtype, gravity=gravity)
    w.upload(B.POS, case.pos)
    w.upload(B.QUAT, case.quat)
    w.upload(B.LVEL, np.zeros((case.n, 3)))
    w.upload(B.AVEL, np.zeros((case.n, 3)))
    if case.hull is not None:
        w.set_convex_hull(case.hull)
        if faces:
            w.set_convex_hull_faces(rs.cube_planes())
    w.upload(B.SIDES, case.sides)
    w.upload_geom_type(case.gtype)
    if case.statics:
        w.set_static_boxes(case.statics)
    if plane is not None:
        w.set_plane(*plane, enable=True)
    return w


def _held(w, case, dtype, plane=rs.PLANE, alive=None, faces=True):
    """the reference's scene from what the device holds"""
    has_hull = case.hull is not None and faces
    return rr.Scene(dtype, w.download(B.POS), w.download(B.QUAT), w.download(B.SIDES), case.gtype, alive,
                    case.hull if has_hull else None, rs.cube_planes() if has_hull else None, case.statics, plane)


def _cast(w, rays, form, mask=B.RAY_ALL):
    w.set_ray_form(form)
    return w.ray_cast(rays[:, 0:3], rays[:, 3:6], rays[:, 6], mask)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _check(ref, got, what):
    bad, worst = rr.compare(ref, got[0], got[1])
    print(f"{what}: {int(ref.band.sum())} of {len(ref.band)} rays in the band; worst depth / pos / normal {worst[0]:.3f} / {worst[1]:.3f} / {worst[2]:.3f} tolerances")
    assert not bad, what + ": " + "; ".join(bad)


_CASES = rs.cases()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(_CASES))
def test_every_form_matches_the_reference_and_the_other_forms(name, dtype):
    case, n_rays, near = _CASES[name]
    rays = rs.make_rays(case, n_rays, rs.SEED, far=not near).astype(dtype)
    with _world(case, dtype) as w:
        ref = rr.cast(_held(w, case, dtype), rays)
        lane = _cast(w, rays, LANE)
        _check(ref, lane, f"{name} {dtype} lane")
        assert _same(lane, _cast(w, rays, BRUTE)), "lane != brute"
        assert _same(lane, _cast(w, rays, WAVE)), "lane != wave"
        for form, counts in ((LANE, (1, 63, 64, 65)), (WAVE, (1, 3, 65))):
            for k in counts:
                sub = _cast(w, rays[n_rays - k:], form)            # (the aimed rays sit at the end)
                assert np.array_equal(sub[0], lane[0][n_rays - k:]) and np.array_equal(sub[1], lane[1][n_rays - k:]), (form, k)
        w.set_ray_form(B.RAY_FORM_AUTO)
        assert _same(lane, w.ray_cast(rays[:, 0:3], rays[:, 3:6], rays[:, 6]))
    assert ref.band.mean() <= (0.002 if near else 0.05)
    if name == "mixed192":
        ids = lane[0]
        assert (ids != B.RAY_MISS).mean() >= 0.4
        g = case.gtype[ids[ids >= 0]]
        counts = {"sphere": int((g == rr.GEOM_SPHERE).sum()), "box": int((g == rr.GEOM_BOX).sum()), "convex": int((g == rr.GEOM_CONVEX).sum()),
                  "static": int((ids <= -3).sum()), "plane": int((ids == B.RAY_PLANE).sum())}
        assert min(counts.values()) >= 20, counts


@pytest.mark.parametrize("dtype", DTYPES)
def test_ray_cast_device_with_torch_buffers_equals_ray_cast(dtype):
    import torch
    case, n_rays, _ = _CASES["mixed70"]
    rays = rs.make_rays(case, 300, 5).astype(dtype)
    with _world(case, dtype) as w:
        for form in (LANE, WAVE):
            host = _cast(w, rays, form)
            t_rays = torch.from_numpy(rays).cuda()
            t_ids = torch.full((300,), 77, dtype=torch.int32, device="cuda")
            t_hits = torch.zeros((300, 7), dtype=t_rays.dtype, device="cuda")
            torch.cuda.synchronize()
            w.ray_cast_device(t_rays.data_ptr(), 300, t_ids.data_ptr(), t_hits.data_ptr())
            w.synchronize()
            assert np.array_equal(t_ids.cpu().numpy(), host[0]) and np.array_equal(t_hits.cpu().numpy(), host[1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_stacked_column_and_degenerate_walks(dtype):
    """40 boxes in one (x,z) column (the buckets grow past 8) under vertical rays from above and from below; rays along the grid's
    axes, vertical rays, and origins at exact multiples of the cell (spheres of radius 0.4: the cell is exactly 1)"""
    rng = np.random.default_rng(3)
    col = sc.column(40)
    k = 64
    xz = np.concatenate([0.1 + 0.3 * rng.uniform(-1, 1, size=(k, 2)), rng.uniform(-2, 2, size=(k, 2))])
    down = np.concatenate([xz[:, :1], np.full((2 * k, 1), 30.0), xz[:, 1:], np.tile([0.0, -1.0, 0.0, 40.0], (2 * k, 1))], 1)
    up = down.copy(); up[:, 1] = -0.75; up[:, 4] = 2.0
    rays = np.concatenate([down, up]).astype(dtype)
    with _world(col, dtype) as w:
        ref = rr.cast(_held(w, col, dtype), rays)
        lane = _cast(w, rays, LANE)
        _check(ref, lane, f"column {dtype}")
        assert _same(lane, _cast(w, rays, WAVE)) and _same(lane, _cast(w, rays, BRUTE))
        assert (lane[0][:k] >= 0).sum() >= k // 2 and (lane[0][2 * k:3 * k] >= 0).sum() >= k // 4
    case = sc.torus_clusters(2, 0)
    dirs = np.array([[1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, 0, -1], [0, -1, 0], [0, 1, 0], [1, 0, 1], [-1, 0, 1], [1, -0.25, 0], [0, -0.25, -1],
                     [0.0, -1.0, 1e-30], [1e-30, -1.0, 0.0]], np.float64)
    org = np.array([[x, y, z] for x in (-2.0, 0.0, 1.0, 2.0, 32.0, 33.0) for y in (0.25, 0.5, 2.0) for z in (-1.0, 0.0, 1.0, 2.0, 3.0)], np.float64)
    rays = np.array([[*o, *d, 48.0] for o in org for d in dirs]).astype(dtype)
    with _world(case, dtype) as w:
        ref = rr.cast(_held(w, case, dtype), rays)
        lane = _cast(w, rays, LANE)
        _check(ref, lane, f"grid-aligned rays {dtype}")
        assert _same(lane, _cast(w, rays, WAVE)) and _same(lane, _cast(w, rays, BRUTE))
        assert (lane[0] >= 0).sum() >= 100


@pytest.mark.parametrize("dtype", DTYPES)
def test_long_rays_give_the_hit_of_short_ones(dtype):
    case, n_rays, _ = _CASES["mixed192"]
    rays = rs.make_rays(case, 2048, 9).astype(dtype)
    rays[:, 6] = 100.0
    far = rays.copy(); far[:, 6] = 1e9
    with _world(case, dtype) as w:
        for form in (LANE, WAVE):
            a, b = _cast(w, rays, form), _cast(w, far, form)
            hit = a[0] != B.RAY_MISS
            assert hit.sum() > 1000
            assert np.array_equal(a[0][hit], b[0][hit]) and np.array_equal(a[1][hit], b[1][hit])
            assert (b[1][~hit, 6] > 100.0).all()               # what 100 m did not reach lies further out, or nowhere
            nowhere = b[0] == B.RAY_MISS
            assert (b[1][nowhere, 6] == np.dtype(dtype).type(1e9)).all() and (b[1][nowhere, 3:6] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_masks_invisible_slots_and_ghost_slots(dtype):
    case = rs.mixed_case(192, seed=12)
    rng = np.random.default_rng(4)
    gtype = case.gtype.copy()
    gtype[rng.random(case.n) < 0.15] = rr.GEOM_NONE                  # slots without a geom: their data is as live as anyone's
    case = sc.Case("holes", case.pos, case.quat, case.sides, gtype, case.hull, case.statics)
    alive = rng.random(case.n) >= 0.15
    rays = rs.make_rays(sc.Case("all", case.pos, case.quat, case.sides, np.maximum(gtype, 1), case.hull, case.statics), 2048, 6).astype(dtype)
    with _world(case, dtype) as w:
        w.upload_body_flags(np.where(alive, B.BODY_ALIVE, B.BODY_KINEMATIC).astype(np.uint8))
        scene = _held(w, case, dtype, alive=alive)
        seen = (gtype != rr.GEOM_NONE) & alive
        for mask in (B.RAY_ALL, B.RAY_SPHERES, B.RAY_BOXES, B.RAY_CONVEX, B.RAY_STATIC, B.RAY_PLANE_BIT, B.RAY_BOXES | B.RAY_PLANE_BIT, 0):
            ref = rr.cast(scene, rays, mask)
            lane = _cast(w, rays, LANE, mask)
            _check(ref, lane, f"mask {mask} {dtype}")
            assert _same(lane, _cast(w, rays, BRUTE, mask)) and _same(lane, _cast(w, rays, WAVE, mask))
            ids = lane[0]
            assert seen[ids[ids >= 0]].all(), "a slot without a geom or without DMX_BODY_ALIVE was hit"
            allowed = {m: ok for m, ok in ((B.RAY_SPHERES, rr.GEOM_SPHERE), (B.RAY_BOXES, rr.GEOM_BOX), (B.RAY_CONVEX, rr.GEOM_CONVEX)) if mask & m}
            assert np.isin(gtype[ids[ids >= 0]], list(allowed.values())).all()
            assert (mask & B.RAY_STATIC) or not (ids <= -3).any()
            assert (mask & B.RAY_PLANE_BIT) or not (ids == B.RAY_PLANE).any()
            if mask == 0:
                assert (ids == B.RAY_MISS).all()
            elif mask in (B.RAY_SPHERES, B.RAY_BOXES, B.RAY_CONVEX, B.RAY_STATIC, B.RAY_PLANE_BIT):
                assert (ids != B.RAY_MISS).sum() >= 20, mask
        # ghost slots [n_active, n) are as visible as anyone
        full = _cast(w, rays, LANE)
        w.set_active_count(96)
        assert _same(full, _cast(w, rays, LANE)) and _same(full, _cast(w, rays, WAVE))
        assert (full[0] >= 96).sum() >= 20


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_hull_without_faces_is_invisible(dtype):
    case, _, _ = _CASES["mixed70"]
    rays = rs.make_rays(case, 1024, 8).astype(dtype)
    with _world(case, dtype, faces=False) as w:
        ref = rr.cast(_held(w, case, dtype, faces=False), rays)
        lane = _cast(w, rays, LANE)
        _check(ref, lane, f"no faces {dtype}")
        assert _same(lane, _cast(w, rays, BRUTE))
        ids = lane[0]
        assert not (case.gtype[ids[ids >= 0]] == rr.GEOM_CONVEX).any() and (ids >= 0).sum() > 100


@pytest.mark.parametrize("dtype", DTYPES)
def test_casts_see_the_state_after_every_enqueued_tick(dtype):
    case, _, _ = _CASES["mixed192"]
    rays = rs.make_rays(case, 2048, 10).astype(dtype)
    with _world(case, dtype, gravity=(0.0, -9.8, 0.0)) as w:
        w.upload(B.LVEL, np.tile([0.5, 0.0, -0.25], (case.n, 1)))
        before = _cast(w, rays, LANE)
        _check(rr.cast(_held(w, case, dtype), rays), before, f"before {dtype}")
        w.step(np.dtype(dtype).type(H), 10)                            # enqueued; the slabs swap
        after = _cast(w, rays, LANE)
        again = _cast(w, rays, LANE)
        assert _same(after, again)
        assert not _same(before, after)
        _check(rr.cast(_held(w, case, dtype), rays), after, f"after {dtype}")
        assert _same(after, _cast(w, rays, WAVE)) and _same(after, _cast(w, rays, BRUTE))
        # an upload is seen too
        pos = w.download(B.POS); pos[:, 1] += 0.5
        w.upload(B.POS, pos)
        moved = _cast(w, rays, LANE)
        _check(rr.cast(_held(w, case, dtype), rays), moved, f"moved {dtype}")
        assert _same(moved, _cast(w, rays, BRUTE))


@pytest.mark.parametrize("dtype", DTYPES)
def test_casts_see_the_state_after_single_launch_ticks(dtype):
    """dmxBatchStepJoints ticks of a small world run as one launch that writes the state itself: the next cast must see it"""
    rng = np.random.default_rng(12)
    n = 24
    sides = np.zeros((n, 3)); sides[:, 0] = 0.4
    case = sc.Case("small", rng.uniform([-2, 0, -2], [2, 1, 2], size=(n, 3)), sc._ident_quats(n), sides, np.full(n, rr.GEOM_SPHERE, np.uint8))
    rays = rs.make_rays(case, 512, 3).astype(dtype)
    with _world(case, dtype, gravity=(0.0, -9.8, 0.0)) as w:
        w.upload(B.LVEL, np.tile([1.0, 0.0, 0.5], (n, 1)))
        before = _cast(w, rays, WAVE)
        for _ in range(6):
            w.step_joints(H, np.zeros(0, B.CONTACT_JOINT_DTYPE))
        after = _cast(w, rays, WAVE)
        st = w.small_tick_stats()
        assert st["small"] + st["general"] == 6 and st["small"] > 0, st
        assert not _same(before, after)
        _check(rr.cast(_held(w, case, dtype), rays), after, f"after single-launch ticks {dtype}")
        assert _same(after, _cast(w, rays, BRUTE)) and _same(after, _cast(w, rays, LANE))


def _run(scene_loader, dtype, ticks, every, rays, between):
    """`ticks` single-tick dmxBatchStep calls; before every `every`-th one: a cast ("cast"), the settling of an open chunk that a
    cast begins with and nothing else ("settle": dmxBatchSynchronize), or nothing ("none")"""
    w = scene_loader()
    h = np.dtype(dtype).type(H)
    n_cast = 0
    for t in range(ticks):
        if t % every == 0 and between == "cast":
            w.set_ray_form((LANE, WAVE)[n_cast % 2])
            ids, _ = w.ray_cast(rays[:, 0:3], rays[:, 3:6], rays[:, 6])
            n_cast += int((ids != B.RAY_MISS).sum() > 0)
        elif t % every == 0 and between == "settle":
            w.synchronize()
        w.step(h, 1)
    w.synchronize()
    out = (w.state(), w.collision_stats(), n_cast)
    w.close()
    return out


def _same_states(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[0], b[0]))


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_cast_leaves_nothing_a_tick_can_tell(dtype, lazy, monkeypatch):
    """The smoke scene (256 boxes dropped on the plane, 90 ticks) and 192 tumbling boxes that take exact ticks, with a cast every 3
    ticks and without: the same states and the same collision statistics.

    What "without" has to mean.  A cast begins by settling the chunk dmxBatchStep may have left open (its violation flag is read; a
    violation rolls the chunk back and replays it) -- it has to: until then the slab may hold a state that will be rolled back.
    Every entry point that observes the batch does the same, and WHEN a chunk is settled shows in the statistics, casts or no casts:
    the smoke scene settled every 3 ticks takes all 90 ticks on the fast path with 14 zone builds; left alone it runs one chunk of 32
    and one of 58 ticks, the second is rolled back and replayed exactly (32 fast, 58 exact ticks, 3 builds).  Same states, bit for bit.
    So:  lazy = False (DMX_LAZY_CHUNKS=0: every dmxBatchStep reads its chunk's flag before it returns, nothing is ever left open):
    casts against no casts, states and statistics equal;  lazy = True (the default): casts against a run that calls
    dmxBatchSynchronize -- which settles and does nothing else -- where the other casts, states and statistics equal, and against
    a run left alone, states equal."""
    if lazy:
        monkeypatch.delenv("DMX_LAZY_CHUNKS", raising=False)
    else:
        monkeypatch.setenv("DMX_LAZY_CHUNKS", "0")
    smoke = pkg.scenes.box_grid(16, 16, seed=1, y_range=(0.6, 1.5), spin=True, box_mass=True).astype(dtype)

    def load_smoke():
        w = pkg.BatchWorld(smoke.n, dtype=dtype)
        w.load_scene(smoke)
        return w
    boxes = sc.tumbling_boxes(192, 7)

    def load_boxes():
        w = _world(boxes, dtype, plane=(0.0, 1.0, 0.0, -2.0), gravity=(0.0, -9.8, 0.0))
        w.upload(B.MASS, np.ones((boxes.n, 1))); w.upload(B.INERTIA, np.ones((boxes.n, 3)))
        return w
    rng = np.random.default_rng(2)
    smoke_rays = np.concatenate([rng.uniform([-13, 0.2, -13], [13, 3, 13], size=(512, 3)), rng.normal(size=(512, 3)), np.full((512, 1), 20.0)], 1).astype(dtype)
    for name, load, ticks, rays in (("smoke", load_smoke, 90, smoke_rays), ("boxes", load_boxes, 30, rs.make_rays(boxes, 512, 4).astype(dtype))):
        cast, alone = _run(load, dtype, ticks, 3, rays, "cast"), _run(load, dtype, ticks, 3, rays, "none")
        print(f"{name} {dtype} lazy={lazy}: with casts {cast[1]}; left alone {alone[1]}")
        assert cast[2] == ticks // 3
        assert _same_states(cast, alone), name
        if lazy:
            settled = _run(load, dtype, ticks, 3, rays, "settle")
            assert _same_states(cast, settled) and cast[1] == settled[1], (name, cast[1], settled[1])
        else:
            assert cast[1] == alone[1], (name, cast[1], alone[1])
        if name == "boxes":
            assert alone[1]["careful_ticks"] > 0


def test_arguments():
    lib = pkg._lib.load()
    with pkg.BatchWorld(64, dtype="float32") as w:
        buf = (C.c_float * 7)(0, 1, 0, 0, -1, 0, 5)
        ids = (C.c_int32 * 1)(5)
        hits = (C.c_float * 7)()
        assert lib.dmxBatchRayCast(w.h, 0, None, None, None, B.RAY_ALL) == 0
        assert lib.dmxBatchRayCastDevice(w.h, 0, None, None, None, B.RAY_ALL) == 0
        EINVAL = -3
        assert lib.dmxBatchRayCast(w.h, 1, None, ids, hits, B.RAY_ALL) == EINVAL
        assert lib.dmxBatchRayCast(w.h, 1, buf, None, hits, B.RAY_ALL) == EINVAL
        assert lib.dmxBatchRayCast(w.h, 1, buf, ids, None, B.RAY_ALL) == EINVAL
        assert lib.dmxBatchRayCast(None, 1, buf, ids, hits, B.RAY_ALL) == EINVAL
        assert lib.dmxBatchRayCast(w.h, -1, buf, ids, hits, B.RAY_ALL) == EINVAL
        assert lib.dmxBatchRayCastDevice(w.h, 1, None, None, None, B.RAY_ALL) == EINVAL
        assert lib.dmxBatchSetRayForm(w.h, 4) == EINVAL and lib.dmxBatchSetRayForm(w.h, -1) == EINVAL
        # an empty world: a miss with the end point; with a plane: the plane
        assert lib.dmxBatchRayCast(w.h, 1, buf, ids, hits, B.RAY_ALL) == 0
        assert ids[0] == B.RAY_MISS and list(hits) == [0.0, -4.0, 0.0, 0.0, 0.0, 0.0, 5.0]
        w.set_plane(0.0, 1.0, 0.0, -1.0)
        assert lib.dmxBatchRayCast(w.h, 1, buf, ids, hits, B.RAY_ALL) == 0
        assert ids[0] == B.RAY_PLANE and list(hits) == [0.0, -1.0, 0.0, 0.0, 1.0, 0.0, 2.0]
        # invalid rays: a miss and zeros
        bad = np.array([[0, 1, 0, 0, 0, 0, 5], [0, 1, 0, 0, -1, 0, 0], [0, 1, 0, 0, -1, 0, -2], [0, 1, 0, 0, -1, 0, np.inf],
                        [0, 1, 0, np.nan, -1, 0, 5], [0, 1, 0, 0, -1, 0, np.nan], [0, 1, 0, np.inf, 0, 0, 5]], np.float32)
        for form in (LANE, WAVE, BRUTE):
            w.set_ray_form(form)
            got = w.ray_cast(bad[:, 0:3], bad[:, 3:6], bad[:, 6])
            assert (got[0] == B.RAY_MISS).all() and (got[1] == 0).all()
