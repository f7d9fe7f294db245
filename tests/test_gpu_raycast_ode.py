"""The ODE face of the ray cast (include/ode/ode.h: dCreateRay, dGeomRaySet, dCollide with a ray), through ctypes on both ODE
libraries (dReal = double and dReal = float): the closed-form cases of tests/test_ray_reference.py, exact in both."""
import ctypes as C
import os

import pytest

from __graft_entry__ import load_package, ROOT

pkg = load_package()
pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "rl-ode-physics_amd")
LIBS = [("libode_mi355.so", C.c_double), ("libode_mi355_single.so", C.c_float)]


def _bind(libname, real):
    pkg._lib.load()
    lib = C.CDLL(os.path.join(PKG, libname))

    class ContactGeom(C.Structure):
        _fields_ = [("pos", real * 4), ("normal", real * 4), ("depth", real), ("g1", C.c_void_p), ("g2", C.c_void_p),
                    ("side1", C.c_int), ("side2", C.c_int)]
    P = C.c_void_p
    for name, res, args in (("dCreateRay", P, [P, real]), ("dGeomRaySet", None, [P] + [real] * 6), ("dGeomRayGet", None, [P, P, P]),
                            ("dGeomRaySetLength", None, [P, real]), ("dGeomRayGetLength", real, [P]), ("dCreateBox", P, [P] + [real] * 3),
                            ("dCreateSphere", P, [P, real]), ("dCreatePlane", P, [P] + [real] * 4), ("dGeomSetPosition", None, [P] + [real] * 3),
                            ("dGeomDestroy", None, [P]), ("dGeomGetClass", C.c_int, [P]), ("dSimpleSpaceCreate", P, [P]), ("dSpaceDestroy", None, [P]),
                            ("dCollide", C.c_int, [P, P, C.c_int, P, C.c_int])):
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    return lib, ContactGeom


def _collide(lib, CG, a, b):
    c = CG()
    n = lib.dCollide(a, b, 1, C.byref(c), C.sizeof(CG))
    return n, c


@pytest.mark.parametrize("libname,real", LIBS)
def test_ray_against_box_sphere_and_plane(libname, real):
    lib, CG = _bind(libname, real)
    ray = lib.dCreateRay(None, 10.0)
    assert ray and lib.dGeomGetClass(ray) == 5 and lib.dGeomRayGetLength(ray) == 10.0
    sphere, box, plane = lib.dCreateSphere(None, 1.0), lib.dCreateBox(None, 2.0, 2.0, 2.0), lib.dCreatePlane(None, 0.0, 2.0, 0.0, 0.0)
    lib.dGeomSetPosition(sphere, 0.0, 0.0, 0.0)
    lib.dGeomSetPosition(box, 0.0, 0.0, 0.0)
    lib.dGeomRaySet(ray, -3.0, 0.0, 0.0, 4.0, 0.0, 0.0)                  # the direction is normalised
    start, d = (real * 4)(), (real * 4)()
    lib.dGeomRayGet(ray, start, d)
    assert list(start)[:3] == [-3.0, 0.0, 0.0] and list(d)[:3] == [1.0, 0.0, 0.0]
    for g in (sphere, box):
        for a, b in ((ray, g), (g, ray)):                               # either order: g1 is the ray
            n, c = _collide(lib, CG, a, b)
            assert n == 1 and c.depth == 2.0 and list(c.pos)[:3] == [-1.0, 0.0, 0.0] and list(c.normal)[:3] == [-1.0, 0.0, 0.0]
            assert c.g1 == ray and c.g2 == g
        lib.dGeomRaySet(ray, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0)               # from the centre: the far side, the normal against the ray
        n, c = _collide(lib, CG, ray, g)
        assert n == 1 and c.depth == 1.0 and list(c.pos)[:3] == [1.0, 0.0, 0.0] and list(c.normal)[:3] == [-1.0, 0.0, 0.0]
        lib.dGeomRaySet(ray, -3.0, 0.0, 0.0, 1.0, 0.0, 0.0)
        lib.dGeomRaySetLength(ray, 1.75)                                 # a quarter short
        assert _collide(lib, CG, ray, g)[0] == 0 and _collide(lib, CG, g, ray)[0] == 0
        lib.dGeomRaySetLength(ray, 10.0)
    lib.dGeomRaySet(ray, 0.5, 2.0, 0.5, 0.0, -1.0, 0.0)                  # the plane y = 0 from above and from below
    n, c = _collide(lib, CG, ray, plane)
    assert n == 1 and c.depth == 2.0 and list(c.pos)[:3] == [0.5, 0.0, 0.5] and list(c.normal)[:3] == [0.0, 1.0, 0.0]
    lib.dGeomRaySet(ray, 0.5, -2.0, 0.5, 0.0, 1.0, 0.0)
    n, c = _collide(lib, CG, plane, ray)
    assert n == 1 and c.depth == 2.0 and list(c.normal)[:3] == [0.0, -1.0, 0.0] and c.g1 == ray and c.g2 == plane
    lib.dGeomRaySet(ray, 0.5, 2.0, 0.5, 1.0, 0.0, 0.0)                   # parallel
    assert _collide(lib, CG, ray, plane)[0] == 0
    ray2 = lib.dCreateRay(None, 1.0)
    assert _collide(lib, CG, ray, ray2)[0] == 0
    for g in (ray, ray2, sphere, box, plane):
        lib.dGeomDestroy(g)                                              # a ray is destroyed like any geom


@pytest.mark.parametrize("libname,real", LIBS)
def test_a_ray_cannot_join_a_space(libname, real, capfd):
    lib, _ = _bind(libname, real)
    space = lib.dSimpleSpaceCreate(None)
    assert lib.dCreateRay(space, 1.0) is None
    assert "dCreateRay" in capfd.readouterr().err
    lib.dSpaceDestroy(space)
