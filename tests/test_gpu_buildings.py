"""Buildings in the whole-g-point pipeline (tsx_pprts_set_buildings / tsx_pprts_get_buildings / tsx_pprts_set_abso_in_buildings)
against the oracle's restatement of the reference pipeline composed with a NumPy restatement of the reference's four buildings
routines (src/pprts.F90, line numbers at each function below):

    alloc_coeff_* -> patch -> explicit_edir -> setup_b_* -> override -> solve -> calc_flx_div -> get_result -> face fluxes

Albedos are multiples of 0.25, so that albedo / streams is exact in real32 and device and restatement hold the same numbers.
Tolerances against the oracle are the ones tests/test_gpu_pipeline.py uses for the same quantities (solar: 2e-4 of the field's
maximum for edn / eup / edir / abso; thermal: 1e-7 for the fluxes, 1e-6 for abso); the face arrays are fluxes and inherit the
flux tolerance.

Scenes: the reference's own 6 x 6 x 3 known-answer scene with one full box at glob_box (i, j, k) = (3, 3, 2)
(tests/test_buildings/test_buildings.F90:157-158); a 6 x 6 x 4 scene with a roof only, a two-cell wall and a RIGHT and a FRONT face
on the last column / row (their dofs wrap); and 4 x 4 x 3 with default tolerances for the scan preconditioner: the rule in
tsx_prepare_ksp (tsx_api.hip) wants fp32 directions (rtol >= 1e-7), xm even and >= 2, ym even on a periodic rank and Nz <= 256 --
2 x 2 x 1 satisfies it, but a building there is its own neighbour on every side; 4 x 4 x 3 is the smallest even grid on which a full
box has a free cell on each of its six sides."""
import ctypes

import numpy as np
import pytest

import test_gpu_pipeline as _pipe
from oracle import oracle as O
from tenstream_amd import _lib, lut
from tenstream_amd.pprts import PprtsSolver, face_index

TOP, BOT, LEFT, RIGHT, REAR, FRONT = range(1, 7)   # PPRTS_*_FACE, src/boxmc_geometry.F90:46-51
SOLAR_TOL, SOLAR_ABSO_TOL = 2e-4, 2e-4             # tests/test_gpu_pipeline.py::test_solar_pipeline_matches_oracle
THERMAL_TOL, THERMAL_ABSO_TOL = 1e-7, 1e-6         # tests/test_gpu_pipeline.py::test_thermal_pipeline_matches_oracle


# ---- NumPy restatement of the reference ---------------------------------------------------------------------------------------------
def ind_1d_to_nd(sizes, ind):
    """src/helper_functions.fypp:2392-2414 (1-based, first dimension fastest)"""
    offs = np.concatenate([[1], np.cumprod(sizes[:-1])])
    nd = [0] * len(sizes)
    nd[-1] = (ind - 1) // offs[-1] + 1
    for k in range(len(sizes) - 2, -1, -1):
        nd[k] = ((ind - 1) % offs[k + 1]) // offs[k] + 1
    return [int(v) for v in nd]


def _dims(solver):
    """(ntop, nside, dtop, dside, top_div, side_div): src/pprts.F90:332-349, 413-425; diffuse area dividers are 1 (:250-251)"""
    return (2, 4, 1, 1, 1, 1) if solver == "3_10" else (8, 4, 4, 2, 4, 2)


def _inward(q):
    return q % 2 == 1   # is_inward = [F, T, F, T, ...] on every face group


def _group(face, ntop, nside):
    """(offset of the face's dof group, dofs in it, streams)"""
    if face in (TOP, BOT):
        return 0, ntop, ntop // 2
    return (ntop, nside, nside // 2) if face in (LEFT, RIGHT) else (ntop + nside, nside, nside // 2)


def _leaving_inward(face):
    return face in (BOT, RIGHT, FRONT)


def patch_dir2dir(t, faces, shape):
    """set_buildings_coeff of alloc_coeff_dir2dir, src/pprts.F90:3194-3212"""
    Nz, Nx, Ny = shape
    t = t.copy()
    for f in faces:
        _, k, i, j = ind_1d_to_nd([6, Nz, Nx, Ny], f)
        t[j - 1, i - 1, k - 1, :] = 0.0
    return t


def patch_diff2diff(c, faces, albedo, shape, solver):
    """set_buildings_coeff of alloc_coeff_diff2diff, src/pprts.F90:3579-3677; c[j, i, k, dst * D + src]"""
    Nz, Nx, Ny = shape
    ntop, nside = _dims(solver)[:2]
    D = ntop + 2 * nside
    c = c.copy()
    for f, alb in zip(faces, albedo):
        face, k, i, j = ind_1d_to_nd([6, Nz, Nx, Ny], f)
        v = c[j - 1, i - 1, k - 1].reshape(D, D)   # v[dst, src]
        off, n, streams = _group(face, ntop, nside)
        for idst in range(n):
            if _inward(idst) == _leaving_inward(face):
                v[off + idst, :] = 0.0
                for isrc in range(n):
                    if _inward(isrc) != _leaving_inward(face):
                        v[off + idst, off + isrc] = alb / streams
    return c


def _dof_home(face, k, i, j, Nx, Ny):
    """0-based (k, i, j) the reference addresses the face's dofs at: k + 1 / i + 1 / j + 1 for BOT / RIGHT / FRONT; the ghost column of
    the single periodic rank is column 0 (halo_reduce_5pt, src/pprts.F90:4676; the entry has no other contributor)"""
    return (k + (face == BOT), (i + (face == RIGHT)) % Nx, (j + (face == FRONT)) % Ny)


def override_b(b, faces, albedo, planck, lsolar, edir, dz, dx, dy, shape, solver):
    """set_buildings_reflection / set_buildings_emission, src/pprts.F90:4669-4672, 4989-5145; b[j, i, level, dof], edir[j, i, level, s]"""
    Nz, Nx, Ny = shape
    ntop, nside, dtop, dside = _dims(solver)[:4]
    b = b.copy()
    for m, (f, alb) in enumerate(zip(faces, albedo)):
        face, k, i, j = ind_1d_to_nd([6, Nz, Nx, Ny], f)
        k, i, j = k - 1, i - 1, j - 1
        off, n, streams = _group(face, ntop, nside)
        kk, ii, jj = _dof_home(face, k, i, j, Nx, Ny)
        if lsolar:
            s0, ns = (0, dtop) if face in (TOP, BOT) else ((dtop, dside) if face in (LEFT, RIGHT) else (dtop + dside, dside))
            v = 0.0
            for isrc in range(s0, s0 + ns):
                v = v + edir[jj, ii, kk, isrc] * alb / streams
        else:
            if planck is None:
                continue
            area = dx * dy if face in (TOP, BOT) else (dy if face in (LEFT, RIGHT) else dx) * dz[j, i, k]
            v = area * (np.pi * planck[m] * (1.0 - alb)) / streams
        for q in range(n):
            if _inward(q) == _leaving_inward(face):
                b[jj, ii, kk, off + q] = v
    return b


def face_fluxes(faces, lsolar, mu, edir_wm2, ediff_wm2, shape, solver):
    """fill_buildings_arr, src/pprts.F90:6011-6247 (no -pprts_fill_1D_side_walls); inputs are restore_solution's W/m2 arrays"""
    Nz, Nx, Ny = shape
    ntop, nside, dtop, dside, top_div, side_div = _dims(solver)
    fe, fi, fo = (np.zeros(len(faces)) for _ in range(3))
    for m, f in enumerate(faces):
        face, k, i, j = ind_1d_to_nd([6, Nz, Nx, Ny], f)
        kk, ii, jj = _dof_home(face, k - 1, i - 1, j - 1, Nx, Ny)
        if lsolar:
            s0, ns, div = (0, dtop, top_div) if face in (TOP, BOT) else ((dtop, dside, side_div) if face in (LEFT, RIGHT)
                                                                          else (dtop + dside, dside, side_div))
            fe[m] = (edir_wm2[jj, ii, kk, s0:s0 + ns] * mu).sum() / div
        off, n, _ = _group(face, ntop, nside)
        for q in range(n):
            v = ediff_wm2[jj, ii, kk, off + q] * (mu if lsolar else 1.0)
            if _inward(q) == _leaving_inward(face):
                fo[m] += v
            else:
                fi[m] += v
    return fe, fi, fo   # diffuse area dividers are 1


def oracle_with_buildings(P, I, faces, albedo, planck_faces, edirTOA, lsolar, planck=None, abso_val=None):
    """tests/test_gpu_pipeline.py::_oracle_pipeline with the four patches in place"""
    F = P.fields
    Nz, Nx, Ny = P.Nz, P.Nx, P.Ny
    shape = (Nz, Nx, Ny)
    solver = I["solver"]
    S, D = (3, 10) if solver == "3_10" else (8, 16)
    lay, dlay, sun = O.layout(solver, Nz, Nx, Ny), O.dir_layout(solver), O.suninfo(P.phi0, P.theta0)
    Ld = O.make_lut(lut.diffuse_axes(solver), lut.synthetic_diffuse_table(solver))
    c0 = O.alloc_coeff_diff2diff(Ld, F["kabs"], F["ksca"], F["g"], F["dz"], I["dx"], P.l1d)
    c = patch_diff2diff(c0, faces, albedo, shape, solver)
    out = dict(diff2diff=c, diff2diff_unpatched=c0)
    if lsolar:
        LT, LS = O.make_lut(I["dax"], I["Tdir"]), O.make_lut(I["dax"], I["Sdir"])
        t = patch_dir2dir(O.alloc_coeff_dir(LT, True, F["kabs"], F["ksca"], F["g"], F["dz"], I["dx"], sun, P.l1d, S=S, D=D), faces, shape)
        sd = O.alloc_coeff_dir(LS, False, F["kabs"], F["ksca"], F["g"], F["dz"], I["dx"], sun, P.l1d, S=S, D=D)   # dir2diff: untouched
        rt, at, _ = O.default_tolerances(Nx, Ny, Nz + 1)
        edir, di = O.explicit_edir(lay, dlay, sun, t, P.l1d, F["a33"], edirTOA, I["dx"], I["dy"], rtol=rt, atol=at)
        assert di["converged"]
        b = O.setup_b_solar(lay, dlay, sun, sd, P.l1d, F["a13"], F["a23"], F["albedo"], edir)
        out.update(dir2dir=t, edir=edir)
    else:
        edir, t, sd = None, None, None
        b = O.setup_b_thermal(lay, c, P.l1d, F["a11"], F["a12"], F["albedo"], planck, F["kabs"], F["dz"], I["dx"], I["dy"])
    b = override_b(b, faces, albedo, planck_faces, lsolar, edir, F["dz"], I["dx"], I["dy"], shape, solver)
    x, info = O.solve_ilu(lay, c, P.l1d, F["a11"], F["a12"], F["albedo"], b, rtol=1e-10, atol=1e-30, maxit=3000)
    assert info["reason"] == 2
    abso = O.calc_flx_div(lay, dlay, sun, t, sd, c, P.l1d, F["a11"], F["a12"], F["kabs"], F["dz"], I["dx"], I["dy"], edir, x,
                          None if lsolar else b)
    ediff_wm2 = O.scale_diff(lay, F["dz"], I["dx"], I["dy"], True, x)
    edir_wm2 = O.scale_dir(lay, dlay, F["dz"], I["dx"], I["dy"], True, edir) if lsolar else None
    redn, reup, rabso, redir = O.get_result(lay, dlay, sun, lsolar, edir_wm2, ediff_wm2, abso)
    fe, fi, fo = face_fluxes(faces, lsolar, sun.mu, edir_wm2, ediff_wm2, shape, solver)
    out.update(b=b, edn=redn, eup=reup, abso=rabso, redir=redir, f_edir=fe, f_in=fi, f_out=fo)
    return out


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def scene(name):
    """(Nx, Ny, Nz, faces, albedo per face)"""
    if name in ("box", "scan"):
        Nx, Ny, Nz = (6, 6, 3) if name == "box" else (4, 4, 3)
        i, j, k = (3, 3, 2) if name == "box" else (2, 3, 2)
        faces = face_index(Nz, Nx, Ny, k, i, j, np.arange(1, 7))
        albedo = np.array([0.5, 0.25, 0.75, 0.0, 1.0, 0.5])
    else:   # "partial": a roof only, a two-cell wall, a RIGHT and a FRONT face on the last column and row
        Nx, Ny, Nz = 6, 6, 4
        faces = np.array([face_index(Nz, Nx, Ny, 3, 2, 2, TOP), face_index(Nz, Nx, Ny, 3, 4, 4, LEFT), face_index(Nz, Nx, Ny, 4, 4, 4, LEFT),
                          face_index(Nz, Nx, Ny, 2, Nx, 3, RIGHT), face_index(Nz, Nx, Ny, 4, 5, Ny, FRONT)])
        albedo = np.array([0.25, 0.5, 0.75, 0.5, 1.0])
    return Nx, Ny, Nz, np.asarray(faces, dtype=np.int64), albedo


def _setup(name, solver, phi0=200.0, theta0=40.0):
    Nx, Ny, Nz, faces, albedo = scene(name)
    P, I = _pipe._setup(Nx, Ny, Nz, phi0, theta0, solver=solver)   # the cloudy synthetic field and LUTs of the pipeline tests
    return P, I, faces, albedo


def _planck_field(Nx, Ny, Nz):
    return np.linspace(2.0, 6.0, Nz + 1)[None, None, :] * np.ones((Ny, Nx, 1))


def _close(got, want, tol, what):
    err, ref = np.abs(got - want).max(), max(np.abs(want).max(), 1e-30)
    print(f"{what}: max |diff| {err:.3e}, max |want| {ref:.3e}, bound {tol * ref:.3e}")
    assert err <= tol * ref, what


# ---- 1. CPU: the restatement itself ---------------------------------------------------------------------------------------------------
def test_face_index_round_trips():
    rng = np.random.default_rng(3)
    for Nz, Nx, Ny in ((3, 6, 6), (4, 5, 7), (1, 2, 2)):
        for _ in range(50):
            f, k, i, j = rng.integers(1, 7), rng.integers(1, Nz + 1), rng.integers(1, Nx + 1), rng.integers(1, Ny + 1)
            assert ind_1d_to_nd([6, Nz, Nx, Ny], face_index(Nz, Nx, Ny, k, i, j, f)) == [f, k, i, j]
        assert face_index(Nz, Nx, Ny, 1, 1, 1, "top") == 1 and face_index(Nz, Nx, Ny, Nz, Nx, Ny, "front") == 6 * Nz * Nx * Ny
    got = face_index(3, 6, 6, 2, 3, 3, np.arange(1, 7))
    assert list(got) == [face_index(3, 6, 6, 2, 3, 3, f) for f in range(1, 7)]
    with pytest.raises(ValueError):
        face_index(3, 6, 6, 4, 1, 1, 1)


class _HostMirror:
    """what oracle_with_buildings reads of a PprtsSolver, without a device: clear air, no delta scaling needed"""

    def __init__(self, Nz, Nx, Ny, phi0, theta0, fields):
        self.Nz, self.Nx, self.Ny, self.phi0, self.theta0, self.fields = Nz, Nx, Ny, phi0, theta0, fields
        self.l1d = np.zeros(Nz, dtype=np.uint8)


@pytest.mark.parametrize("box_albedo,Ag", [(0.0, 0.0), (0.5, 1.0)])
def test_restatement_reproduces_the_references_known_answers(box_albedo, Ag):
    """tests/test_buildings/test_buildings.F90:151-207 and :209-260 on the oracle pipeline, sun overhead: edir at the box's bottom face and
    in the cell below is exactly 0, the roof sees the full beam, and outgoing == (edir + incoming) * albedo on every face."""
    Nx, Ny, Nz, faces, _ = scene("box")
    albedo = np.full(6, box_albedo)
    solver = "3_10"
    z = np.zeros((Ny, Nx, Nz))
    F = dict(kabs=z + 1e-12, ksca=z + 1e-12, g=z, dz=z + 50.0, albedo=np.full((Ny, Nx), Ag), a11=z, a12=z, a13=z, a23=z, a33=z,
             planck_srfc=None)
    P = _HostMirror(Nz, Nx, Ny, 0.0, 0.0, F)
    dax = lut.direct_axes()
    Tdir, Sdir = lut.synthetic_direct_tables(dax, solver)
    I = dict(dx=100.0, dy=100.0, dax=dax, Tdir=Tdir, Sdir=Sdir, solver=solver)
    R = oracle_with_buildings(P, I, faces, albedo, None, 1.0, True)
    assert R["redir"][2, 2, 2] == 0.0 and R["redir"][2, 2, 3] == 0.0   # bottom of the box (k = 2 -> level 2), beneath it
    assert R["f_edir"][BOT - 1] == 0.0
    assert R["f_edir"][TOP - 1] == R["redir"][2, 2, 1] > 0.0
    scale = max(np.abs(R["f_edir"]).max(), np.abs(R["f_in"]).max())
    assert np.abs((R["f_edir"] + R["f_in"]) * albedo - R["f_out"]).max() <= 1e-9 * scale   # the oracle solve stops at rtol 1e-10
    if box_albedo == 0.0:
        assert np.all(R["f_out"] == 0.0)


# ---- 2. the patch kernels -------------------------------------------------------------------------------------------------------------
def _dedup_mode(P):
    P.core.dedup_info()
    return P.core.dedup_mode


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["box", "partial"])
@pytest.mark.parametrize("solver", ["3_10", "8_16"])
def test_patched_coefficients_equal_the_restatement(gpu, solver, name):
    P, I, faces, albedo = _setup(name, solver)
    shape = (P.Nz, P.Nx, P.Ny)
    P.set_optical_properties(0.15, I["kabs"], I["ksca"], I["g"], I["dz"])
    plain = P.core.get_coeffs()
    P.set_buildings(faces, albedo)
    P.set_optical_properties(0.15, I["kabs"], I["ksca"], I["g"], I["dz"])
    got = P.core.get_coeffs()
    want = patch_diff2diff(plain, faces, albedo, shape, solver)
    assert np.array_equal(got, want)
    touched = want != plain
    assert touched.any() and np.array_equal(got[~touched], plain[~touched])   # untouched entries bit-identical to the handle without buildings
    ntop, nside = _dims(solver)[:2]
    vals = set(np.unique(got[touched]))
    allowed = {0.0} | {float(np.float32(a / s)) for a in albedo for s in (ntop // 2, nside // 2)}
    assert vals <= allowed, vals - allowed   # zeroed entries exactly 0, reflected ones exactly float32(albedo / streams)
    info = P.solve(1000.0)
    assert info.reason in (2, 3)
    t = P.get_field("dir2dir")
    for f in faces:
        _, k, i, j = ind_1d_to_nd([6, *shape], int(f))
        assert np.all(t[j - 1, i - 1, k - 1] == 0.0)
    R = oracle_with_buildings(P, I, faces, albedo, None, 1000.0, True)
    assert np.array_equal(t, R["dir2dir"])
    P.close()


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["3_10", "8_16"])
def test_equal_building_blocks_share_one_entry(gpu, solver):
    """A homogeneous atmosphere, two building cells with the same face and albedo, a third with another albedo: sharing stays on and
    the distinct blocks are the background's, the pair's and the third one's."""
    Nx, Ny, Nz = 6, 6, 4
    P, I = _pipe._setup(Nx, Ny, Nz, 200.0, 40.0, solver=solver)
    one = np.ones((Ny, Nx, Nz))
    args = (0.1, 1e-4 * one, 2e-3 * one, 0.3 * one, 50.0 * one)
    P.set_optical_properties(*args)
    P.solve(1000.0)
    on, n0 = P.core.dedup_info()
    assert on and n0 == 1
    faces = [face_index(Nz, Nx, Ny, 2, 2, 2, TOP), face_index(Nz, Nx, Ny, 3, 5, 4, TOP), face_index(Nz, Nx, Ny, 3, 2, 5, TOP)]
    P.set_buildings(faces, [0.5, 0.5, 0.25])
    P.set_optical_properties(*args)
    info = P.solve(1000.0)
    assert info.reason in (2, 3)
    on, n = P.core.dedup_info()
    assert on and n == 3, (on, n)
    P.close()


# ---- 3. + 4. the pipeline against oracle + restatement, and the identities on the device result ----------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["box", "partial"])
@pytest.mark.parametrize("solver", ["3_10", "8_16"])
def test_solar_pipeline_with_buildings_matches_oracle(gpu, monkeypatch, solver, name):
    monkeypatch.setenv("TSX_NO_RETRY", "1")   # a first attempt that fails is reported, not repeated: reason 2 = converged without the retry
    P, I, faces, albedo = _setup(name, solver)
    P.set_buildings(faces, albedo)
    P.set_optical_properties(0.15, I["kabs"], I["ksca"], I["g"], I["dz"])
    info = P.solve(1000.0, rtol=1e-10, atol=1e-30, maxit=3000)
    assert info.reason == 2
    R = oracle_with_buildings(P, I, faces, albedo, None, 1000.0, True)
    edn, eup, abso, edir = P.get_result()
    for got, want, what in ((edn, R["edn"], "edn"), (eup, R["eup"], "eup"), (edir, R["redir"], "edir")):
        _close(got, want, SOLAR_TOL, what)
    _close(abso, R["abso"], SOLAR_ABSO_TOL, "abso")
    fe, fi, fo = P.get_buildings()
    flux = max(np.abs(R["edn"]).max(), np.abs(R["redir"]).max())   # the face arrays are fluxes of this scene
    for got, want, what in ((fe, R["f_edir"], "face edir"), (fi, R["f_in"], "face incoming"), (fo, R["f_out"], "face outgoing")):
        print(what, got, want)
        assert np.abs(got - want).max() <= SOLAR_TOL * flux, what
    # check_buildings_energy_balance on the device result
    assert np.abs((fe + fi) * albedo - fo).max() <= SOLAR_TOL * flux
    if name == "box":
        assert fe[BOT - 1] == 0.0   # the beam leaving a full box
        assert edir[2, 2, 2] == 0.0   # ... at the box's bottom level; the cell beneath is lit through its sides by this slanted sun
                                      # (beneath the box the beam is 0 only with the sun overhead: the CPU known-answer test)
    P.close()


@pytest.mark.gpu
@pytest.mark.parametrize("with_planck", [True, False])
@pytest.mark.parametrize("name", ["box", "partial"])
@pytest.mark.parametrize("solver", ["3_10", "8_16"])
def test_thermal_pipeline_with_buildings_matches_oracle(gpu, monkeypatch, solver, name, with_planck):
    monkeypatch.setenv("TSX_NO_RETRY", "1")
    P, I, faces, albedo = _setup(name, solver, 0.0, 0.0)
    planck = _planck_field(P.Nx, P.Ny, P.Nz)
    pf = np.linspace(3.0, 8.0, len(faces)) if with_planck else None
    P.set_buildings(faces, albedo, planck=pf)
    P.set_optical_properties(0.1, I["kabs"], I["ksca"], I["g"], I["dz"], planck=planck)
    info = P.solve(0.0, rtol=1e-10, atol=1e-30, maxit=3000)
    assert info.reason == 2
    R = oracle_with_buildings(P, I, faces, albedo, pf, 0.0, False, planck=planck)
    _close(P.get_field("b"), R["b"], 1e-13, "b")
    edn, eup, abso, _ = P.get_result()
    _close(edn, R["edn"], THERMAL_TOL, "edn")
    _close(eup, R["eup"], THERMAL_TOL, "eup")
    _close(abso, R["abso"], THERMAL_ABSO_TOL, "abso")
    fe, fi, fo = P.get_buildings()
    assert np.all(fe == 0.0)   # no solar solve: zeros
    flux = np.abs(R["edn"]).max()
    for got, want, what in ((fi, R["f_in"], "face incoming"), (fo, R["f_out"], "face outgoing")):
        print(what, got, want)
        assert np.abs(got - want).max() <= THERMAL_TOL * max(flux, np.abs(want).max()), what
    if with_planck:
        bal = fo - albedo * fi - np.pi * pf * (1.0 - albedo)
        assert np.abs(bal).max() <= THERMAL_TOL * max(flux, np.abs(fo).max())
    P.close()


# ---- 5. state -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["3_10", "8_16"])
def test_albedo_change_detach_and_call_order(gpu, monkeypatch, solver):
    monkeypatch.setenv("TSX_NO_RETRY", "1")
    P, I, faces, albedo = _setup("box", solver)
    args = (0.15, I["kabs"], I["ksca"], I["g"], I["dz"])
    opts = dict(rtol=1e-10, atol=1e-30, maxit=3000, zero_guess=True)
    P.set_optical_properties(*args)
    P.solve(1000.0, **opts)
    plain = [a.copy() for a in P.get_result()]
    # changing only the albedos between two coefficient sets gives the second scene's result (no stale grouping)
    second = albedo[::-1].copy()
    P.set_buildings(faces, albedo)
    P.set_optical_properties(*args)
    P.solve(1000.0, **opts)
    first_res = [a.copy() for a in P.get_result()]
    P.set_buildings(faces, second)
    P.set_optical_properties(*args)
    P.solve(1000.0, **opts)
    got = P.get_result()
    fresh, _, _, _ = _setup("box", solver)
    fresh.set_buildings(faces, second)
    fresh.set_optical_properties(*args)
    fresh.solve(1000.0, **opts)
    for a, b_, c in zip(got, fresh.get_result(), first_res):
        assert np.array_equal(a, b_)
    assert not np.array_equal(got[1], first_res[1])
    for a, b_ in zip(P.get_buildings(), fresh.get_buildings()):
        assert np.array_equal(a, b_)
    fresh.close()
    # set_buildings after set_optical_properties: the solve wants new optical properties
    P.set_buildings(faces, albedo)
    with pytest.raises(_lib.TsxError) as e:
        P.solve(1000.0)
    assert e.value.code == 4   # TSX_ERR_STATE
    # set_abso_in_buildings overwrites exactly the building cells
    P.set_optical_properties(*args)
    P.solve(1000.0, **opts)
    ref_abso = P.get_result()[2].copy()
    P.set_abso_in_buildings(-7.5)
    abso = P.get_result()[2]
    mask = np.zeros(abso.shape, dtype=bool)
    mask[2, 2, 1] = True
    assert np.all(abso[mask] == -7.5) and np.array_equal(abso[~mask], ref_abso[~mask])
    P.set_abso_in_buildings(None)
    assert np.array_equal(P.get_result()[2], ref_abso)
    # detaching reproduces the no-buildings result bit for bit
    P.set_buildings([], [])
    with pytest.raises(_lib.TsxError) as e:
        P.solve(1000.0)
    assert e.value.code == 4
    P.set_optical_properties(*args)
    P.solve(1000.0, **opts)
    for a, b_ in zip(P.get_result(), plain):
        assert np.array_equal(a, b_)
    P.close()


@pytest.mark.gpu
def test_unsupported_combinations_and_invalid_face_lists(gpu):
    Nx, Ny, Nz, faces, albedo = scene("box")
    def _code(fn):
        with pytest.raises(_lib.TsxError) as e:
            fn()
        return e.value.code, str(e.value)

    P, I = _pipe._setup(Nx, Ny, Nz, 200.0, 40.0)
    # TSX_ERR_ARG = 1, naming the first offending entry
    c, msg = _code(lambda: P.set_buildings([faces[0], 6 * Nz * Nx * Ny + 1], 0.5))
    assert c == 1 and "iface[1]" in msg
    c, msg = _code(lambda: P.set_buildings([faces[0], 0], 0.5))
    assert c == 1 and "iface[1]" in msg
    c, msg = _code(lambda: P.set_buildings([faces[0], faces[1], faces[0]], 0.5))
    assert c == 1 and "iface[2]" in msg and "twice" in msg
    c, msg = _code(lambda: P.set_buildings(faces[:3], [0.5, 1.25, -0.1]))
    assert c == 1 and "albedo[1]" in msg
    c, msg = _code(lambda: P.set_buildings(faces[:2], [0.5, float("nan")]))
    assert c == 1 and "albedo[1]" in msg
    with pytest.raises(_lib.TsxError):
        P.get_buildings()   # nothing attached, nothing solved
    # a face in a layer that is solved 1-D: TSX_ERR_UNSUPPORTED = 5 at set_optical_properties
    P.set_buildings(faces, albedo)
    dz = I["dz"].copy()
    dz[:, :, :2] = 400.0
    c, msg = _code(lambda: P.set_optical_properties(0.1, I["kabs"], I["ksca"], I["g"], dz))
    assert c == 5 and "1-D" in msg
    # the caller-derived whole-g-point entry cannot carry the patch
    P.close()
    # collapsed handle, 1-D solver handle, more than one rank
    Pc, _ = _pipe._setup(Nx, Ny, Nz + 1, 200.0, 40.0, collapseindex=2)
    assert _code(lambda: Pc.set_buildings(faces, albedo))[0] == 5
    Pc.close()
    P1 = PprtsSolver(Nz, Nx, Ny, 100.0, 100.0, 200.0, 40.0, solver_1d="twostream")
    assert _code(lambda: P1.set_buildings(faces, albedo))[0] == 5
    P1.close()
    P2 = PprtsSolver(Nz, Nx, Ny, 100.0, 100.0, 200.0, 40.0, xs=0, ys=0, glob_xm=2 * Nx, glob_ym=Ny, rank=0, nranks=2,
                     neighbors=(1, 1, 0, 0))
    assert _code(lambda: P2.set_buildings(faces, albedo))[0] == 5
    P2.close()
    # switched on after the buildings were attached: refused when the optical properties arrive
    P3, I3 = _pipe._setup(Nx, Ny, Nz, 200.0, 40.0)
    P3.set_buildings(faces, albedo)
    P3.set_1d_solver("twostream")
    assert _code(lambda: P3.set_optical_properties(0.1, I3["kabs"], I3["ksca"], I3["g"], I3["dz"]))[0] == 5
    P3.close()


# ---- 6. hostile memory ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("lsolar", [True, False])
def test_buildings_on_poisoned_memory(gpu, lsolar):
    """in the manner of tests/test_gpu_pool_hostile.py: the case runs twice in one process, TSX_POOL_POISON unset and then 0xFF; the
    results must be bit-identical and no red zone damaged"""
    from test_gpu_pool_hostile import POISON, pool_check

    def case():
        out = []
        for solver in ("3_10", "8_16"):
            P, I, faces, albedo = _setup("partial", solver, 200.0 if lsolar else 0.0, 40.0 if lsolar else 0.0)
            planck = None if lsolar else _planck_field(P.Nx, P.Ny, P.Nz)
            for alb in (albedo, albedo[::-1].copy()):   # a second coefficient set: same faces, other albedos
                P.set_buildings(faces, alb, planck=None if lsolar else np.linspace(3.0, 8.0, len(faces)))
                P.set_optical_properties(0.15, I["kabs"], I["ksca"], I["g"], I["dz"], planck=planck)
                info = P.solve(1000.0 if lsolar else 0.0)
                assert info.reason in (2, 3)
                out += [P.core.get_coeffs(), P.get_field("b"), *P.get_result()[:3], *P.get_buildings()]
                if lsolar:
                    out.append(P.get_field("dir2dir"))
            P.close()
        return out

    assert pool_check(gpu, reset=1)[1] == 0
    runs = []
    for poison in (None, POISON):
        with pytest.MonkeyPatch.context() as mp:
            if poison is None:
                mp.delenv("TSX_POOL_POISON", raising=False)
            else:
                mp.setenv("TSX_POOL_POISON", poison)
            runs.append(case())
            if poison is not None:
                st = pool_check(gpu, reset=1)
                assert st[1] == 0, f"red zones damaged: {st}"
    for q, (a, b_) in enumerate(zip(*runs)):
        assert np.array_equal(a, b_), f"output {q} differs on poisoned memory"
        assert np.isfinite(b_).all()


# ---- 7. the default preconditioner (scan kernels, flow launch) meets building blocks ----------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("lsolar", [True, False])
@pytest.mark.parametrize("solver", ["3_10", "8_16"])
def test_scan_preconditioner_with_buildings(gpu, monkeypatch, solver, lsolar):
    monkeypatch.setenv("TSX_NO_RETRY", "1")
    P, I, faces, albedo = _setup("scan", solver, 200.0 if lsolar else 0.0, 40.0 if lsolar else 0.0)
    planck = None if lsolar else _planck_field(P.Nx, P.Ny, P.Nz)
    pf = None if lsolar else np.linspace(3.0, 8.0, len(faces))
    args = (0.15, I["kabs"], I["ksca"], I["g"], I["dz"])
    P.core.log_enable(True)
    P.set_optical_properties(*args, planck=planck)
    plain = P.solve(1000.0 if lsolar else 0.0)
    assert plain.reason in (2, 3) and P.core.pc_info()[2]   # the scan kernels ran
    t_plain = P.core.log_get()["set_optprop"][1]
    P.set_buildings(faces, albedo, planck=pf)
    P.set_optical_properties(*args, planck=planck)
    info = P.solve(1000.0 if lsolar else 0.0, zero_guess=True)
    assert info.reason in (2, 3)   # converged without the retry
    assert P.core.pc_info()[2]
    t_bld = P.core.log_get()["set_optprop"][1] - t_plain
    print(f"BUILDINGS_REPORT {solver} {'solar' if lsolar else 'thermal'} {P.Nx}x{P.Ny}x{P.Nz}: iterations without / with buildings "
          f"{plain.niter} / {info.niter}; set_optprop device ms without / with {t_plain:.4f} / {t_bld:.4f}")
    R = oracle_with_buildings(P, I, faces, albedo, pf, 1000.0 if lsolar else 0.0, lsolar, planck=planck)
    edn, eup, abso, _ = P.get_result()
    # default tolerances here (rtol 1e-5): the bound of the solar pipeline test, whose direct sweep stops at the same rtol
    _close(edn, R["edn"], SOLAR_TOL, "edn")
    _close(eup, R["eup"], SOLAR_TOL, "eup")
    P.close()
