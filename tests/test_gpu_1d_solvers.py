"""The 1-D routes of solve_pprts on the device: twostream, schwarz and the two-stream initial guess (tsx_1d.hip;
tsx_pprts_set_1d_solver, tsx_pprts_guess_from_2str).

The oracle knows neither routine, so this file restates delta_eddington_twostream (src/twostream.F90:50-184: the banded system,
assembled densely and solved with numpy.linalg.solve), adding_delta_eddington_twostream (:335-390) and schwarzschild
(src/schwarzschild.F90:81-135, use_legendre) in NumPy, one column at a time.  Eddington coefficients and B_eff come from the oracle's
bindings, which are pinned to the reference's vectors; Gauss-Legendre nodes from numpy.polynomial.legendre.leggauss mapped to (0, 1).

Bounds.  eps = 2^-52.  Recurrence paths (adding, schwarz), per column: |delta| <= 32 * levels * eps * max|column| -- one rounding
per operation, at most 32 operations per level, accumulated linearly.  Banded path: 8 * cond(A) * eps * max|column| with cond(A) of
the restatement's own matrix.  "max|column|" is the largest flux of the column (S, Edn, Eup together: every flux of a column is
a sum of products of the others); the absorption of a layer is a difference of those fluxes divided by dz, so its scale is that
maximum divided by the layer's dz.  The observed maxima (profiles/r07/onedim_parity.txt) are written to the file TSX_PARITY_OUT names, when set."""
import ctypes
import os

import numpy as np
import pytest

from oracle import oracle as O
from tenstream_amd import _lib, lut, synthetic
from tenstream_amd.pprts import PprtsSolver

EPS = np.finfo(np.float64).eps
DX = DY = 100.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement (one column; layers top first) ------------------------------------------------------------------------------
def edd(dtau, w0, g, mu0):
    a = np.array([O.eddington_coeff_ec(float(t), float(w), float(q), float(mu0)) for t, w, q in zip(dtau, w0, g)])
    return a[:, 0], a[:, 1], a[:, 2], a[:, 3], a[:, 4]   # a11, a12, a13, a23, a33


def ref_twostream_banded(dtau, w0, g, mu0, incSolar, albedo, planck=None, planck_srfc=None):
    """delta_eddington_twostream (src/twostream.F90:50-184).  Returns S, Edn, Eup and the matrix."""
    ke = len(dtau)
    ke1, N = ke + 1, 2 * (ke + 1)
    a11, a12, a13, a23, a33 = edd(dtau, w0, g, mu0)
    S = np.zeros(ke1)
    if mu0 > 0:
        S[0] = incSolar
        for k in range(ke):
            S[k + 1] = S[k] * a33[k]
    B = np.zeros(N)
    A = np.eye(N)
    for k in range(ke):          # rows 2k: Eup(k), 2k + 1: Edn(k)   (0-based levels)
        B[2 * k] = S[k] * a13[k]
        B[2 * k + 3] = S[k] * a23[k]
    B[1] = 0.0
    B[2 * ke] = S[ke] * albedo
    if planck is not None:
        for k in range(ke):
            emis = max(0.0, min(1.0, 1.0 - a11[k] - a12[k])) * np.pi
            B[2 * k] += emis * O.B_eff(planck[k + 1], planck[k], dtau[k])
            B[2 * k + 3] += emis * O.B_eff(planck[k], planck[k + 1], dtau[k])
        B[2 * ke] += (planck[ke] if planck_srfc is None else planck_srfc) * (1.0 - albedo) * np.pi
    for k in range(ke):
        A[2 * k, 2 * k + 2] = -a11[k]
        A[2 * k, 2 * k + 1] = -a12[k]
        A[2 * k + 3, 2 * k + 1] = -a11[k]
        A[2 * k + 3, 2 * k + 2] = -a12[k]
    A[2 * ke, 2 * ke + 1] = -albedo
    x = np.linalg.solve(A, B)
    return S, x[1::2].copy(), x[0::2].copy(), A


def ref_twostream_adding(dtau, w0, g, mu0, S0, Ag):
    """adding_delta_eddington_twostream (src/twostream.F90:335-390)"""
    ke = len(dtau)
    a11, a12, a13, a23, a33 = edd(dtau, w0, g, mu0)
    R, T, Tdir, Sdir = (np.zeros(ke) for _ in range(4))
    Edir, Edn, Eup = (np.zeros(ke + 1) for _ in range(3))
    Edir[0] = S0
    R[0], T[0], Tdir[0], Sdir[0] = a12[0], a11[0], a33[0], a23[0]
    for k in range(ke - 1):
        R[k + 1] = a12[k + 1] + (R[k] * a11[k + 1] * a11[k + 1]) / (1 - R[k] * a12[k + 1])
        T[k + 1] = T[k] * a11[k + 1] / (1 - R[k] * a12[k + 1])
        Tdir[k + 1] = Tdir[k] * a33[k + 1]
        Sdir[k + 1] = (a11[k + 1] * Sdir[k] + Tdir[k] * a13[k + 1] * R[k] * a11[k + 1]) / (1 - R[k] * a12[k + 1]) + Tdir[k] * a23[k + 1]
    for k in range(ke, 0, -1):
        Edir[k] = Tdir[k - 1] * Edir[0]
    Edn[ke] = (Sdir[ke - 1] + Tdir[ke - 1] * R[ke - 1] * Ag) / (1 - R[ke - 1] * Ag) * Edir[0]
    Eup[ke] = Ag * (Edn[ke] + Edir[ke])
    for t in range(ke - 1, 0, -1):   # level t from level t + 1
        den = 1 - R[t - 1] * a12[t]
        Edn[t] = (R[t - 1] * a11[t] * Eup[t + 1] + Edir[0] * Sdir[t - 1] + Edir[t] * a13[t] * R[t - 1]) / den
        Eup[t] = (a11[t] * Eup[t + 1] + Edir[0] * Sdir[t - 1] * a12[t] + Edir[t] * a13[t]) / den
    Eup[0] = a11[0] * Eup[1] + a13[0] * Edir[0]
    return Edir, Edn, Eup


def gauss01(nmu):
    x, w = np.polynomial.legendre.leggauss(nmu)
    return 0.5 * (x + 1.0), 0.5 * w


def ref_radiance(tau, B_near, B_far, L):
    """schwarzschild_radiance (src/schwarzschild.F90:69-80)"""
    if tau > 1e-3:
        tm1 = np.expm1(-tau)
        return L * (tm1 + 1) + (B_far - B_near) - (B_near - (B_far - B_near) / tau) * tm1
    return (B_near + B_far) * .5 * tau + L * (1.0 - tau)


def ref_schwarz(nmu, dtau, albedo, planck, srfc=None):
    """schwarzschild (src/schwarzschild.F90:81-135), use_legendre"""
    ke = len(dtau)
    Edn, Eup = np.zeros(ke + 1), np.zeros(ke + 1)
    Bs = planck[ke] if srfc is None else srfc
    pts, wis = gauss01(nmu)
    for mu, wi in zip(pts, wis):
        L = 0.0
        for k in range(ke):
            L = ref_radiance(dtau[k] / mu, planck[k], planck[k + 1], L)
            Edn[k + 1] += L * mu * wi
    for mu, wi in zip(pts, wis):
        L = Bs * (1.0 - albedo) + albedo * Edn[ke] * 2
        Eup[ke] += L * mu * wi
        for k in range(ke - 1, -1, -1):
            L = ref_radiance(dtau[k] / mu, planck[k + 1], planck[k], L)
            Eup[k] += L * mu * wi
    return Edn * 2 * np.pi, Eup * 2 * np.pi


# ---- the wrappers twostream / schwarz of src/pprts_1D_solvers.F90 over a whole field ---------------------------------------------
def ref_field(I, c, mu0, edirTOA, lsolar, schwarz=False, nmu=2):
    """Raw inputs I (Ny, Nx, Nz_atm) -> dict(edn, eup, edir (Ny, Nx, Nz+1), abso (Ny, Nx, Nz)) as pprts_get_result hands them out,
    S / Edn / Eup on the atmosphere's levels (before * mu0), per-column cond(A) (banded path) and the flux scale of each column."""
    kabs, ksca, g = synthetic.delta_scale(I["kabs"].copy(), I["ksca"].copy(), I["g"].copy())
    dz = I["dz"]
    Ny, Nx, nza = kabs.shape
    Nz = nza - c + 1
    out = {n: np.zeros((Ny, Nx, Nz + 1)) for n in ("edn", "eup", "edir")}
    out["abso"] = np.zeros((Ny, Nx, Nz))
    atm = {n: np.zeros((Ny, Nx, nza + 1)) for n in ("S", "Edn", "Eup")}
    cond = np.ones((Ny, Nx))
    planck, srfc = I.get("planck"), I.get("planck_srfc")
    for j in range(Ny):
        for i in range(Nx):
            Ag = float(I["albedo"][j, i])
            pl = None if planck is None else planck[j, i]
            sf = None if srfc is None else float(srfc[j, i])
            if schwarz:
                Edn, Eup = ref_schwarz(nmu, dz[j, i] * kabs[j, i], Ag, pl, sf)
                S = np.zeros(nza + 1)
            else:
                kext = kabs[j, i] + ksca[j, i]
                dtau, w0 = dz[j, i] * kext, ksca[j, i] / np.maximum(kext, EPS)
                m0, inc = (mu0, edirTOA) if lsolar else (0.0, 0.0)
                if pl is not None:
                    S, Edn, Eup, A = ref_twostream_banded(dtau, w0, g[j, i], m0, inc, Ag, pl, sf)
                    cond[j, i] = np.linalg.cond(A)
                else:
                    S, Edn, Eup = ref_twostream_adding(dtau, w0, g[j, i], m0, inc, Ag)
            atm["S"][j, i], atm["Edn"][j, i], atm["Eup"][j, i] = S, Edn, Eup
            lev = np.r_[0, np.arange(c, nza + 1)]          # level 0 <- 0, level k >= 1 <- atmk(0) + k
            a = np.arange(c - 1, nza)                      # atmk(k)
            ab = +Edn[a] - Edn[a + 1] - Eup[a] + Eup[a + 1]
            if lsolar:
                ab = ab + S[a] - S[a + 1]
            f = mu0 if lsolar else 1.0
            out["edn"][j, i], out["eup"][j, i], out["edir"][j, i] = Edn[lev] * f, Eup[lev] * f, (S[lev] * f if lsolar else 0.0)
            out["abso"][j, i] = ab / dz[j, i, a] * f
    out.update(atm=atm, cond=cond, dz_solver=dz[:, :, c - 1:],
               scale=np.maximum.reduce([np.abs(atm[n]).max(axis=2) for n in ("S", "Edn", "Eup")]) * (mu0 if lsolar else 1.0))
    return out


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def inputs(Nx, Ny, nza, seed=5, thermal=False, srfc=False, ksca0=False, dz_all=None):
    kabs, ksca, g = synthetic.cloud_field(Nx, Ny, nza, seed=seed)
    kabs *= 20.0
    rng = np.random.default_rng(seed)
    kabs = kabs * (1 + 0.2 * rng.random(kabs.shape)) + 1e-5   # horizontally varying, no transparent layer
    if ksca0:
        ksca = np.zeros_like(ksca)
    dz = np.full((Ny, Nx, nza), 50.0) * (1 + 0.3 * rng.random((Ny, Nx, nza)))
    if dz_all is not None:
        dz = np.full((Ny, Nx, nza), float(dz_all))
    I = dict(kabs=kabs, ksca=ksca, g=g, dz=dz, albedo=0.05 + 0.3 * rng.random((Ny, Nx)))
    if thermal:
        I["planck"] = np.linspace(2.0, 6.0, nza + 1)[None, None, :] * (1 + 0.05 * rng.random((Ny, Nx, 1))) + 0.3 * rng.random((Ny, Nx, nza + 1))
        if srfc:
            I["planck_srfc"] = I["planck"][:, :, -1] * (1.1 + 0.2 * rng.random((Ny, Nx)))
    return I


def branch_clearance(I, nmus=(1, 2, 3, 4)):
    """smallest relative distance of any dtau (B_eff_mu: kext dz / mu of the 2 nodes; schwarzschild_radiance: kabs dz / mu of the
    quadratures used) from the 1e-3 branch points, and the largest w0"""
    kabs, ksca, _ = synthetic.delta_scale(I["kabs"].copy(), I["ksca"].copy(), I["g"].copy())
    d = np.inf
    for nmu in nmus:
        for mu in gauss01(nmu)[0]:
            for tau in (I["dz"] * kabs, I["dz"] * (kabs + ksca)):
                d = min(d, np.abs(tau / mu - 1e-3).min() / 1e-3)
    for tau in (I["dz"] * kabs, I["dz"] * (kabs + ksca)):
        d = min(d, np.abs(tau - 1e-3).min() / 1e-3)
    return d, (ksca / np.maximum(kabs + ksca, EPS)).max()


GRID = (8, 6, 14)   # Nx, Ny, Nz_atm
KINDS = ("solar", "thermal", "thermal_srfc")


def case_inputs(kind, seed=5, **kw):
    return inputs(*GRID, seed=seed, thermal=kind != "solar", srfc=kind == "thermal_srfc", **kw)


# ---- CPU: the yardstick checks itself ------------------------------------------------------------------------------------------------
def test_restated_twostream_passes_the_reference_unit_test():
    """tests/test_twostr/test_twostr.F90: ke = 9, dtau = 1 / ke, w0 = g = .5, mu0 = .5, incSolar = 100, albedo = .1"""
    ke, mu0, inc, alb = 9, .5, 100.0, .1
    dtau, w0, g = np.full(ke, 1.0 / ke), np.full(ke, .5), np.full(ke, .5)
    tol = np.sqrt(EPS)
    S, Edn, Eup, _ = ref_twostream_banded(dtau, w0, g, mu0, inc, alb)
    S2, Edn2, Eup2 = ref_twostream_adding(dtau, w0, g, mu0, inc, alb)
    for s, dn, up in ((S, Edn, Eup), (S2, Edn2, Eup2)):
        assert s[0] == inc
        assert abs(s[ke] - np.exp(-dtau.sum() / mu0) * inc) <= tol * inc
        assert dn[0] == 0 or abs(dn[0]) <= tol
        assert abs(up[ke] - (s[ke] + dn[ke]) * alb) <= tol * abs(up[ke])
    for a, b in ((S, S2), (Edn, Edn2), (Eup, Eup2)):
        assert np.all(np.abs(a - b) <= tol * np.maximum(np.abs(a), 1.0))


@pytest.mark.parametrize("nmu", [1, 2, 5, 16])
def test_restated_schwarzschild_limits(nmu):
    B, ke = 3.7, 6
    pts, wis = gauss01(nmu)
    fac = 2 * np.sum(pts * wis)
    assert abs(fac - 1.0) <= 4 * EPS
    Edn, Eup = ref_schwarz(nmu, np.full(ke, 400.0), 0.0, np.full(ke + 1, B))      # isothermal, optically thick, black ground
    assert abs(Edn[ke] - np.pi * B * fac) <= 1e-13 * np.pi * B and abs(Eup[0] - np.pi * B * fac) <= 1e-13 * np.pi * B
    Edn, Eup = ref_schwarz(nmu, np.zeros(ke), 0.3, np.linspace(1, 5, ke + 1), srfc=2.5)   # empty atmosphere
    assert np.all(Edn == 0) and np.all(np.abs(Eup - np.pi * 2.5 * 0.7) <= 4 * EPS * np.pi * 2.5)


def test_inputs_keep_clear_of_the_branch_points():
    for kind in KINDS:
        for kw in ({}, dict(ksca0=True), dict(dz_all=400.0), dict(dz_all=400.0, ksca0=True)):
            d, w0max = branch_clearance(case_inputs(kind, **kw))
            assert d >= 1e-6 and w0max <= 0.999, (kind, kw, d, w0max)
    d, w0max = branch_clearance(inputs(12, 10, 12, seed=7, dz_all=50.0))
    assert d >= 1e-6 and w0max <= 0.999


def test_abi_surface_has_the_1d_entries():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "tsx.h")).read()
    for sym in ("tsx_pprts_set_1d_solver", "tsx_pprts_guess_from_2str"):
        assert hasattr(lib, sym) and sym in _lib.SYMBOLS and f"int {sym}(" in header
    for name in ("TSX_1D_OFF 0", "TSX_1D_TWOSTREAM 1", "TSX_1D_SCHWARZSCHILD 2"):
        assert f"#define {name}" in header


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
_OBSERVED = {}


def _record(key, ratio):
    _OBSERVED[key] = max(_OBSERVED.get(key, 0.0), float(ratio))
    if os.environ.get("TSX_PARITY_OUT"):
        with open(os.environ["TSX_PARITY_OUT"], "w") as f:
            f.write("# largest |device - restatement| / bound per case (bound: see tests/test_gpu_1d_solvers.py); <= 1 passes\n")
            for k in sorted(_OBSERVED):
                f.write(f"{k}: {_OBSERVED[k]:.3e}\n")


def check_against(ref, got, levels, banded, key):
    edn, eup, abso, edir = got
    fac = (8 * ref["cond"] if banded else 32.0 * levels * np.ones_like(ref["cond"])) * EPS
    bound = (fac * ref["scale"])[:, :, None]
    worst = 0.0
    for name, dev in (("edn", edn), ("eup", eup), ("edir", edir)):
        r = np.abs(dev - ref[name]) / bound
        print(f"{key} {name}: max |delta| / bound = {r.max():.3e}")
        worst = max(worst, r.max())
    r = np.abs(abso - ref["abso"]) / (bound / ref["dz_solver"])
    print(f"{key} abso: max |delta| / bound = {r.max():.3e}")
    worst = max(worst, r.max())
    _record(key, worst)
    assert np.isfinite(worst) and worst <= 1.0, (key, worst)


def run_1d(I, solver, c, mode, lsolar, edirTOA=1000.0, theta0=30.0, nmu=2, **kw):
    Nx, Ny, nza = I["kabs"].shape[1], I["kabs"].shape[0], I["kabs"].shape[2]
    P = PprtsSolver(nza, Nx, Ny, DX, DY, 10.0, theta0, solver=solver, collapseindex=c, solver_1d=mode, nmu=nmu, **kw)
    P.set_optical_properties(I["albedo"], I["kabs"], I["ksca"], I["g"], I["dz"], planck=I.get("planck"), planck_srfc=I.get("planck_srfc"))
    info = P.solve(edirTOA if lsolar else 0.0, lsolar=lsolar)
    return P, info, P.get_result()


@pytest.mark.gpu
@pytest.mark.parametrize("solver,kind,c,force_halo", [(s, k, c, False) for s in ("3_10", "8_16") for k in KINDS for c in (1, 4)]
                         + [("3_10", "solar", 4, True), ("3_10", "thermal", 1, True)])
def test_twostream_kernel_equals_the_restatement(gpu, solver, kind, c, force_halo):
    I = case_inputs(kind)
    lsolar = kind == "solar"
    P, info, got = run_1d(I, solver, c, "twostream", lsolar, **({"force_halo": True} if force_halo else {}))
    assert info.reason == 101 and info.niter == 0
    ref = ref_field(I, c, P.mu0, 1000.0, lsolar)
    check_against(ref, got, GRID[2] + 1, banded=not lsolar, key=f"twostream {solver} {kind} c={c} halo={int(force_halo)}")
    P.close()


@pytest.mark.gpu
@pytest.mark.parametrize("solver,kind,c,nmu", [("3_10", "thermal", 1, 2), ("3_10", "thermal_srfc", 4, 2), ("8_16", "thermal", 4, 3),
                                               ("8_16", "thermal_srfc", 1, 1), ("3_10", "thermal", 1, 16)])
def test_schwarz_kernel_equals_the_restatement(gpu, solver, kind, c, nmu):
    I = case_inputs(kind)
    P, info, got = run_1d(I, solver, c, "schwarzschild", False, nmu=nmu)
    assert info.reason == 102 and info.niter == 0
    ref = ref_field(I, c, P.mu0, 0.0, False, schwarz=True, nmu=nmu)
    check_against(ref, got, GRID[2] + 1, banded=False, key=f"schwarz {solver} {kind} c={c} nmu={nmu}")
    P.close()


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["3_10", "8_16"])
@pytest.mark.parametrize("lsolar", [True, False])
def test_twostream_equals_the_3d_solve_where_every_layer_is_1d(gpu, solver, lsolar):
    """dz / dx > 2 throughout: the columns decouple and the 3-D system's vertical streams obey the two-stream equations.  Solar with
    scattering; thermal with ksca = 0 only, because set_thermal_source feeds B_eff with kabs dz (src/pprts.F90:4869) where twostream
    feeds it kext dz.  1e-8 of the field maximum with the 3-D solve at rtol 1e-10, as tests/test_gpu_config3.py.
    The solar absorption is compared in no case: calc_flx_div takes the direct beam's share in a 1-D layer as
    edir * (1 - exp(-kabs dz / costheta)) (src/pprts.F90:5305-5308), twostream as the divergence of its fluxes, S (1 - a33 - a13 - a23)
    (src/pprts_1D_solvers.F90:220-233); the two differ by the Eddington closure (8.4e-4 of the maximum on this atmosphere, with edn and
    eup equal to 1e-14).  The thermal absorption has no such term and is compared."""
    import test_gpu_pipeline as _pipe

    Nx, Ny, Nz = 8, 6, 10
    P3, J = _pipe._setup(Nx, Ny, Nz, 10.0, 30.0, tall_top=Nz, solver=solver)
    rng = np.random.default_rng(11)
    albedo = 0.05 + 0.9 * rng.random((Ny, Nx))
    ksca = J["ksca"] if lsolar else np.zeros_like(J["ksca"])
    planck = None if lsolar else np.linspace(2.0, 6.0, Nz + 1)[None, None, :] * (1 + 0.05 * rng.random((Ny, Nx, 1)))
    P3.set_optical_properties(albedo, J["kabs"], ksca, J["g"], J["dz"], planck=planck)
    assert P3.l1d.all()
    edir0 = 1000.0 if lsolar else 0.0
    i3 = P3.solve(edir0, lsolar=lsolar, zero_guess=True, rtol=1e-10, atol=1e-30)
    assert i3.reason > 0
    r3 = P3.get_result()
    orc = _pipe._oracle_pipeline(P3, J, albedo, edir0, lsolar, planck=planck, rtol=1e-10)
    P1 = PprtsSolver(Nz, Nx, Ny, DX, DY, 10.0, 30.0, solver=solver, solver_1d="twostream")
    P1.set_optical_properties(albedo, J["kabs"], ksca, J["g"], J["dz"], planck=planck)
    P1.solve(edir0, lsolar=lsolar)
    r1 = P1.get_result()
    names = ("edn", "eup", "edir") if lsolar else ("edn", "eup", "abso")
    for name, a, b in zip(("edn", "eup", "abso", "edir"), r1, r3):
        if name not in names:
            continue
        o = orc["redir" if name == "edir" else name]
        for what, ref in (("3-D device solve", b), ("oracle pipeline", o)):
            rel = np.abs(a - ref).max() / np.abs(ref).max()
            print(f"{solver} lsolar={lsolar} {name} vs {what}: {rel:.3e}")
            assert rel <= 1e-8, (name, what, rel)
    P1.close()
    P3.close()


def _expected_guess(P, I, c, edirTOA, lsolar, solver):
    """twostream's fluxes as src/pprts_1D_solvers.F90:201-218 places them, through the oracle's scale_flx(lWm2 = .false.)"""
    ref = ref_field(I, c, P.mu0, edirTOA, lsolar)
    lay, dlay = O.layout(solver, P.Nz, P.Nx, P.Ny), O.dir_layout(solver)
    S, D = (3, 10) if solver == "3_10" else (8, 16)
    ntop, dtop = (2, 1) if solver == "3_10" else (8, 4)
    lev = np.r_[0, np.arange(c, P.Nz_atm + 1)]
    e = np.zeros(P.core.vec_shape)
    for d in range(ntop):
        e[..., d] = (ref["atm"]["Edn"] if d & 1 else ref["atm"]["Eup"])[:, :, lev] * (1.0 / (ntop // 2))
    ediff = O.scale_diff(lay, ref["dz_solver"], DX, DY, False, e)
    edir = None
    if lsolar:
        ed = np.zeros((P.Ny, P.Nx, P.Nz + 1, S))
        for s in range(dtop):
            ed[..., s] = ref["atm"]["S"][:, :, lev] * 1.0
        edir = O.scale_dir(lay, dlay, ref["dz_solver"], DX, DY, False, ed)
    return ref, ediff, edir


@pytest.mark.gpu
@pytest.mark.parametrize("solver,kind,c", [("3_10", "solar", 1), ("3_10", "thermal", 4), ("8_16", "solar", 4), ("8_16", "thermal_srfc", 1)])
def test_guess_from_2str_fills_every_dof_as_the_reference_does(gpu, solver, kind, c):
    import test_gpu_collapse as _col

    I = case_inputs(kind)
    lsolar = kind == "solar"
    P, _ = _col.solver_for(solver, *GRID, c, phi0=10.0)
    P.set_optical_properties(I["albedo"], I["kabs"], I["ksca"], I["g"], I["dz"], planck=I.get("planck"), planck_srfc=I.get("planck_srfc"))
    P.guess_from_2str(1000.0 if lsolar else 0.0, lsolar=lsolar)
    ref, ediff, edir = _expected_guess(P, I, c, 1000.0, lsolar, solver)
    fac = (32.0 * (GRID[2] + 1) if lsolar else 8 * ref["cond"]) * EPS * np.ones_like(ref["cond"])
    bound = (fac * ref["scale"] / (P.mu0 if lsolar else 1.0) * DX * DY)[:, :, None, None]
    got = P.get_field("ediff")
    r = (np.abs(got - ediff) / bound).max()
    print(f"guess {solver} {kind} c={c} ediff: {r:.3e}")
    assert r <= 1.0
    side = got[..., (2 if solver == "3_10" else 8):]
    assert np.all(side == 0.0)   # solution%ediff = zero (src/pprts_1D_solvers.F90:108) times a face area
    if lsolar:
        r = (np.abs(P.get_field("edir") - edir) / bound).max()
        print(f"guess {solver} {kind} c={c} edir: {r:.3e}")
        assert r <= 1.0
    _record(f"guess {solver} {kind} c={c}", r)
    P.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lsolar", [True, False])
def test_solve_from_the_guess_starts_closer_where_every_layer_is_1d(gpu, lsolar):
    import test_gpu_pipeline as _pipe

    Nx, Ny, Nz = 8, 6, 10
    P, J = _pipe._setup(Nx, Ny, Nz, 10.0, 30.0, tall_top=Nz)
    ksca = J["ksca"] if lsolar else np.zeros_like(J["ksca"])
    planck = None if lsolar else np.linspace(2.0, 6.0, Nz + 1)[None, None, :] * np.ones((Ny, Nx, 1))
    P.set_optical_properties(0.2, J["kabs"], ksca, J["g"], J["dz"], planck=planck)
    e0 = 1000.0 if lsolar else 0.0
    i0 = P.solve(e0, lsolar=lsolar, zero_guess=True, rtol=1e-10, atol=1e-30)
    r0 = [a.copy() for a in P.get_result()]
    # the stop rule is relative to the initial residual (src/pprts.F90:4455-4458), and this guess is the solution up to rounding:
    # stop at the absolute residual the zero-guess solve reached instead
    P.guess_from_2str(e0, lsolar=lsolar)
    i1 = P.solve(e0, lsolar=lsolar, rtol=1e-10, atol=1e-10 * i0.rnorm0)
    r1 = P.get_result()
    print(f"lsolar={lsolar}: rnorm0 zero guess {i0.rnorm0:.3e} ({i0.niter} its), 2str guess {i1.rnorm0:.3e} ({i1.niter} its)")
    assert i1.reason > 0 and i1.rnorm0 < i0.rnorm0
    for a, b in zip(r1[:3], r0[:3]):
        assert np.abs(a - b).max() <= 1e-8 * np.abs(b).max()
    P.close()


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["3_10", "8_16"])
def test_solve_from_the_guess_reaches_the_same_solution_on_a_3d_cloud_field(gpu, solver):
    import test_gpu_pipeline as _pipe

    P, J = _pipe._setup(12, 10, 12, 10.0, 40.0, tall_top=2, seed=7, solver=solver)
    P.set_optical_properties(0.15, J["kabs"], J["ksca"], J["g"], J["dz"])
    i0 = P.solve(1000.0, zero_guess=True, rtol=1e-10, atol=1e-30)
    r0 = [a.copy() for a in P.get_result()]
    P.guess_from_2str(1000.0)
    i1 = P.solve(1000.0, rtol=1e-10, atol=1e-30)
    r1 = P.get_result()
    print(f"{solver} 3-D cloud field: zero guess {i0.niter} its (rnorm0 {i0.rnorm0:.3e}), 2str guess {i1.niter} its (rnorm0 {i1.rnorm0:.3e})")
    assert i1.reason > 0
    for a, b in zip(r1, r0):
        assert np.abs(a - b).max() <= 1e-8 * np.abs(b).max()
    P.close()


@pytest.mark.gpu
def test_semantics_of_the_1d_modes(gpu):
    I = case_inputs("thermal")
    Is = case_inputs("solar")
    # mode 2: schwarz for thermal, twostream for solar (src/pprts.F90:2629-2637); no LUT anywhere
    P, info, got = run_1d(I, "3_10", 1, "schwarzschild", False)
    assert info.reason == 102
    P.set_optical_properties(Is["albedo"], Is["kabs"], Is["ksca"], Is["g"], Is["dz"])
    info = P.solve(1000.0)
    assert info.reason == 101
    ref = ref_field(Is, 1, P.mu0, 1000.0, True)
    check_against(ref, P.get_result(), GRID[2] + 1, banded=False, key="mode 2, solar")
    # a thermal solve without planck is refused with a message
    with pytest.raises(Exception, match="planck"):
        P.solve(0.0, lsolar=False)
    for which in ("b", "ediff", "dir2dir", "dir2diff"):
        with pytest.raises(Exception, match="1-D"):
            P.get_field(which)
    with pytest.raises(Exception):
        P.core.apply(np.zeros(P.core.vec_shape))   # tsx_diff_* on a LUT-less handle: no coefficients
    with pytest.raises(Exception, match="1-D"):
        P.guess_from_2str(1000.0)
    for nmu in (0, 17):
        with pytest.raises(Exception, match="nmu"):
            P.set_1d_solver("schwarzschild", nmu)
    P.close()


@pytest.mark.gpu
def test_switching_the_mode_on_and_off_leaves_the_3d_result_bit_identical(gpu):
    import test_gpu_pipeline as _pipe

    def run(switch):
        P, J = _pipe._setup(10, 8, 8, 20.0, 40.0, tall_top=2)
        if switch:
            P.set_1d_solver("twostream")
            P.set_optical_properties(0.1, J["kabs"], J["ksca"], J["g"], J["dz"])
            P.solve(1000.0)
            P.get_result()
            P.set_1d_solver(None)
            with pytest.raises(Exception):
                P.solve(1000.0)   # the optical properties went with the mode
        P.set_optical_properties(0.1, J["kabs"], J["ksca"], J["g"], J["dz"])
        info = P.solve(1000.0)
        r = [a.copy() for a in P.get_result()]
        P.close()
        return info, r

    (ia, ra), (ib, rb) = run(False), run(True)
    assert ia.niter == ib.niter and ia.reason == ib.reason
    for a, b in zip(ra, rb):
        assert np.array_equal(a, b)


@pytest.mark.gpu
def test_uid_parking_round_trips_a_1d_solution(gpu):
    I, Is = case_inputs("thermal"), case_inputs("solar")
    P, _, r_th = run_1d(I, "3_10", 4, "twostream", False)          # uid 0: thermal
    r_th = [a.copy() for a in r_th]
    P.set_optical_properties(Is["albedo"], Is["kabs"], Is["ksca"], Is["g"], Is["dz"])
    P.solve(1000.0, uid=1)
    r_so = [a.copy() for a in P.get_result()]
    _lib.check(gpu.tsx_pprts_select_solution(P.h, 0))
    for a, b in zip(P.get_result(), r_th):
        assert np.array_equal(a, b)
    _lib.check(gpu.tsx_pprts_select_solution(P.h, 1))
    for a, b in zip(P.get_result(), r_so):
        assert np.array_equal(a, b)
    _lib.check(gpu.tsx_pprts_select_solution(P.h, 5))              # never solved: nothing to hand out
    with pytest.raises(Exception, match="no solution"):
        P.get_result()
    P.close()


@pytest.mark.gpu
def test_log_events_of_a_1d_gpoint(gpu):
    I = case_inputs("thermal")
    Nx, Ny, nza = GRID
    P = PprtsSolver(nza, Nx, Ny, DX, DY, 10.0, 30.0, solver_1d="schwarzschild")
    P.core.log_enable()
    base = P.core.log_get()
    assert "solve_twostream" not in base and "solve_schwarzschild" not in base and len(base) == 11
    P.set_optical_properties(I["albedo"], I["kabs"], I["ksca"], I["g"], I["dz"])
    P.solve(1000.0)
    P.get_result()
    ev = P.core.log_get()
    assert ev["solve_twostream"][0] == 1 and "solve_schwarzschild" not in ev
    assert ev["set_optprop"][0] == 1 and ev["get_result"][0] == 1
    for name in ("solve_Mdiff", "setup_Mdiff", "compute_Edir", "compute_Ediff", "get_coeff_diff2diff", "compute_absorption"):
        assert ev[name][0] == 0, name
    P.set_optical_properties(I["albedo"], I["kabs"], I["ksca"], I["g"], I["dz"], planck=I["planck"])
    P.solve(0.0, lsolar=False)
    ev = P.core.log_get()
    assert ev["solve_schwarzschild"][0] == 1 and ev["solve_twostream"][0] == 1 and len(ev) == 13
    P.close()


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["twostream_solar", "twostream_thermal", "schwarz", "guess"])
def test_1d_paths_on_hostile_memory(gpu, what):
    import test_gpu_collapse as _col
    import test_gpu_pool_hostile as _hos

    def case(mp):
        if what == "guess":
            I = case_inputs("solar")
            P, _ = _col.solver_for("3_10", *GRID, 4, phi0=10.0)
            P.set_optical_properties(I["albedo"], I["kabs"], I["ksca"], I["g"], I["dz"])
            P.guess_from_2str(1000.0)
            P.get_field("ediff")
            P.get_field("edir")
            P.solve(1000.0)
            P.get_result()
        else:
            kind = "solar" if what == "twostream_solar" else "thermal_srfc"
            P, _, _ = run_1d(case_inputs(kind), "8_16", 4, "schwarzschild" if what == "schwarz" else "twostream", kind == "solar")
        P.close()

    _hos.hostile(gpu, case)


# ---- the reference's own C-ABI ---------------------------------------------------------------------------------------------------
_F2C_CHILD = r"""
import ctypes as C, sys, numpy as np
lib = C.CDLL(sys.argv[1])
solver_id, thermal, out = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
Nx = Ny = 3; Nz = 10
I = np.load(sys.argv[5])
i32 = lambda v: C.byref(C.c_int(v)); f64 = lambda v: C.byref(C.c_double(v)); f32 = lambda v: C.byref(C.c_float(v))
p = lambda a: a.ctypes.data_as(C.c_void_p)
hhl = I["hhl"].astype(np.float32)
lib.pprts_f2c_init(0, i32(solver_id), i32(Nz), i32(Nx), i32(Ny), f64(100.0), f64(100.0), p(hhl), f32(180.0), f32(0.0), i32(1))
alb = np.float32(0.1)
fields = [np.ascontiguousarray(I[n], dtype=np.float32) for n in ("kabs", "ksca", "g", "planck")]
lib.pprts_f2c_set_global_optical_properties(Nz, Nx, Ny, C.byref(C.c_float(alb)), p(fields[0]), p(fields[1]), p(fields[2]),
                                            p(fields[3]) if thermal else None)
lib.pprts_f2c_solve.argtypes = [C.c_int, C.c_float]
lib.pprts_f2c_solve(0, 0.0 if thermal else 1.0)
nl, nc = (Nz + 1) * Nx * Ny, Nz * Nx * Ny
r = [np.zeros(n, dtype=np.float32) for n in (nl, nl, nc, nl)]
lib.pprts_f2c_get_result(Nz, Nx, Ny, p(r[0]), p(r[1]), p(r[2]), p(r[3]))
lib.pprts_f2c_destroy(0)
np.savez(out, edn=r[0], eup=r[1], abso=r[2], edir=r[3])
"""


def _ex1_inputs():
    """the grid and the optical properties of examples/pprts (ex_pprts_ex1.F90:37-80, pprts_ex1.F90:76-78): 3 x 3 x 10, dx = dy = dz =
    100, phi0 = 180, theta0 = 0, albedo .1, clear sky dtau 1, w0 .5, g 0, a cloud (dtau 1, w0 .99, g .9) in layer Nlay / 2 + 1 of
    the centre column; as float32, the kind of this ABI"""
    Nx = Ny = 3
    Nz = 10
    dz = 100.0
    kabs = np.full((Ny, Nx, Nz), 1.0 / dz / Nz * 0.5, dtype=np.float32)
    ksca = kabs.copy()
    g = np.zeros((Ny, Nx, Nz), dtype=np.float32)
    kabs[1, 1, Nz // 2] = np.float32(1.0 / dz * 0.01)
    ksca[1, 1, Nz // 2] = np.float32(1.0 / dz * 0.99)
    g[1, 1, Nz // 2] = np.float32(0.9)
    planck = (np.float32(100.0 / np.pi) * (1 + 0.05 * np.arange(Nz + 1, dtype=np.float32))[None, None, :]
              * np.ones((Ny, Nx, 1), dtype=np.float32)).astype(np.float32)
    hhl = (np.float32(dz) * (Nz - np.arange(Nz + 1)).astype(np.float32)).astype(np.float32)
    return dict(kabs=kabs, ksca=ksca, g=g, planck=planck, hhl=hhl)


def _run_f2c(tmp_path, solver_id, thermal, petsc_options=None):
    import subprocess
    import sys

    I = _ex1_inputs()
    np.savez(str(tmp_path / "in.npz"), **I)
    out = str(tmp_path / "out.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("LUT_BASENAME", "PETSC_OPTIONS")}
    env["LUT_BASENAME"] = str(tmp_path / "no_such_tables")   # no LUT files present
    if petsc_options:
        env["PETSC_OPTIONS"] = petsc_options
    lib = os.path.join(ROOT, "tenstream_amd", "lib", "libtsx_f2c.so")
    r = subprocess.run([sys.executable, "-c", _F2C_CHILD, lib, str(solver_id), str(int(thermal)), out, str(tmp_path / "in.npz")],
                       env=env, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.load(out)
    dz = (I["hhl"][:-1].astype(np.float64) - I["hhl"][1:].astype(np.float64))
    J = dict(kabs=I["kabs"].astype(np.float64), ksca=I["ksca"].astype(np.float64), g=I["g"].astype(np.float64),
             dz=np.broadcast_to(dz, I["kabs"].shape).copy(), albedo=np.full((3, 3), float(np.float32(0.1))))
    if thermal:
        J["planck"] = I["planck"].astype(np.float64)
    return got, J


def _check_f2c(got, ref):
    """the ABI hands out float32: half an ulp of the result on top of the fp64 bound"""
    for name in ("edn", "eup", "abso", "edir"):
        want = ref[name]
        err = np.abs(got[name].reshape(want.shape) - want).max()
        print(f"f2c {name}: {err:.3e} (max {np.abs(want).max():.3e})")
        assert err <= 2.0 ** -24 * np.abs(want).max() * 1.01 + 1e-30, name


@pytest.mark.gpu
@pytest.mark.parametrize("thermal", [False, True])
def test_f2c_2str_solver_without_tables_equals_the_restatement(gpu, tmp_path, thermal):
    got, J = _run_f2c(tmp_path, 2, thermal)
    _check_f2c(got, ref_field(J, 1, 1.0, 1.0, not thermal))


@pytest.mark.gpu
def test_f2c_schwarzschild_option_selects_schwarz_for_a_thermal_call(gpu, tmp_path):
    got, J = _run_f2c(tmp_path, 310, True, "-schwarzschild -schwarzschild_Nmu 3")
    _check_f2c(got, ref_field(J, 1, 1.0, 0.0, False, schwarz=True, nmu=3))
