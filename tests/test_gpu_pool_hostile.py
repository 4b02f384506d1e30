"""Every solver path on hostile device memory (the pool's TSX_POOL_POISON mode, tsx_pool.hip).

A piece of the pool that is handed out again keeps what its last user left in it, and a write a few elements past a buffer lands in
the rounding slack or in a neighbour: a kernel that relies on zeros it never wrote, or that reads a slot before writing it, gives
results that depend on what ran before it in the process.  Each case here runs twice in one process -- (a) with the mode unset, on
whatever the pool holds by then, (b) with TSX_POOL_POISON=255: every piece taken or freed is filled with 0xFF bytes (NaN as fp64,
fp32, fp16, bf16 and fp8, -1 as an integer) and carries red zones -- and (b) must be bit-identical to (a), finite, and equal to the
oracle at the tolerance of the existing test of that path (the case bodies are those tests), with no red zone damaged at the end.
Every case takes and frees memory during a solver's life (second coefficient sets, growth of the shared storage, warm-started
second solves, close); multi-rank cases spawn rank processes that inherit the mode and check their own pool before they exit
(test_gpu_multirank._guarded)."""
import ctypes
import gc

import numpy as np
import pytest

import test_gpu_multirank as _mr
import test_gpu_parity as _par
import test_gpu_pipeline as _pipe
import test_gpu_seam as _seam
from oracle import oracle as O
from tenstream_amd import DiffuseSolver, synthetic
from tenstream_amd.pprts import PprtsSolver

pytestmark = pytest.mark.gpu

POISON = "255"
# what the solvers hand back, recorded for the comparison of the two runs (every array argument after the call, and the result)
_RECORDED = {DiffuseSolver: ("apply", "pc_apply", "get_coeffs", "solve", "dir_solve", "setup_b_solar", "setup_b_thermal"),
             PprtsSolver: ("solve", "get_result", "get_field")}


def _flatten(v, out):
    if isinstance(v, np.ndarray):
        out.append(v.copy())
    elif type(v).__module__.startswith("torch"):
        out.append(v.detach().cpu().numpy().copy())
    elif isinstance(v, (list, tuple)):
        for e in v:
            _flatten(e, out)
    elif isinstance(v, dict):
        for k in sorted(v, key=str):
            _flatten(v[k], out)
    elif isinstance(v, (bool, int, float, np.integer, np.floating)):
        out.append(np.asarray(v))
    elif hasattr(v, "res_hist"):   # KspInfo: everything but the timings
        _flatten([v.reason, v.niter, v.rnorm0, v.rnorm, v.res_hist], out)


def _recording(mp, rec):
    def wrap(fn):
        def f(*args, **kw):
            r = fn(*args, **kw)
            _flatten([r, [a for a in args[1:] if not isinstance(a, (int, float, str))], kw], rec)
            return r
        return f

    for cls, names in _RECORDED.items():
        for n in names:
            mp.setattr(cls, n, wrap(getattr(cls, n)))
    real_spawn = _mr._spawn

    def spawn(*a, **kw):   # the rank processes' results, as the parent sees them
        r = real_spawn(*a, **kw)
        _flatten({k: v for k, v in r.items() if not isinstance(k, tuple)}, rec)
        return r

    mp.setattr(_mr, "_spawn", spawn)


def pool_check(gpu, reset=0):
    st = (ctypes.c_int64 * 4)()
    assert gpu.tsx_pool_check(-1, reset, st) == 0
    return [int(v) for v in st]


def hostile(gpu, case, finite=True):
    """case(monkeypatch): one run of a test body.  (a) mode unset, (b) TSX_POOL_POISON=255: bit-identical, finite, zones whole."""
    assert pool_check(gpu, reset=1)[1] == 0
    runs = []
    for poison in (None, POISON):
        rec = []
        with pytest.MonkeyPatch.context() as mp:
            if poison is None:
                mp.delenv("TSX_POOL_POISON", raising=False)
            else:
                mp.setenv("TSX_POOL_POISON", poison)
            _recording(mp, rec)
            case(mp)
            gc.collect()   # solvers a body did not close are freed now, in their run's mode
            if poison is not None:
                st = pool_check(gpu, reset=1)
                assert st[1] == 0, f"red zones damaged: {st[1]} (first: a {st[2]}-byte piece, byte {st[3]} from its end)"
        runs.append(rec)
    a, b = runs
    assert len(a) == len(b) and len(b) > 0
    for q, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype, q
        assert np.array_equal(x, y, equal_nan=True), f"output {q} differs on poisoned memory"
        if finite and y.dtype.kind in "fc":
            assert np.isfinite(y).all(), f"output {q} is not finite"


# ---- operator apply ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,Nx,Ny,Nz,n1d", [("3_10", 7, 5, 3, 2), ("3_10", 3, 3, 1, 0), ("8_16", 5, 6, 5, 1)])
@pytest.mark.parametrize("force_halo", [False, True])
def test_apply_on_poisoned_memory(gpu, solver, Nx, Ny, Nz, n1d, force_halo):
    hostile(gpu, lambda mp: _par.test_apply_matches_oracle(gpu, solver, Nx, Ny, Nz, n1d, force_halo))


def test_apply_fp64_coefficients_on_poisoned_memory(gpu):
    hostile(gpu, lambda mp: _par.test_apply_fp64_coefficients_kept_when_lossy(gpu))


# ---- BiCGStab ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,Nx,Ny,Nz,n1d", [("3_10", 7, 6, 17, 2), ("8_16", 5, 3, 9, 1)])
@pytest.mark.parametrize("pc", [0, 2, 3])
def test_solve_on_poisoned_memory(gpu, solver, Nx, Ny, Nz, n1d, pc):
    hostile(gpu, lambda mp: _par.test_solve_matches_oracle(gpu, solver, Nx, Ny, Nz, n1d, False, pc))


def test_default_tolerances_and_warm_start_on_poisoned_memory(gpu):
    hostile(gpu, lambda mp: _par.test_solve_default_tolerances_and_warm_start(gpu))


@pytest.mark.parametrize("solver,Nx,Ny,Nz,n1d", [("3_10", 7, 5, 17, 2), ("3_10", 6, 4, 33, 1), ("8_16", 5, 3, 9, 1)])
def test_solver_life_on_poisoned_memory(gpu, solver, Nx, Ny, Nz, n1d):
    """One solver takes and frees memory through its life: a first set and solve, a second coefficient set (fp64 kept: lossy), the
    operator and a tight solve on it against the oracle, a warm-started second solve, preconditioner applications, close."""
    import scipy.sparse.linalg as spla

    def case(mp):
        P = synthetic.make_problem(solver, Nx=Nx, Ny=Ny, Nz=Nz, n1d=n1d, seed=Nz)
        lay = O.layout(solver, Nz, Nx, Ny)
        s = DiffuseSolver(solver, Nz, Nx, Ny)
        s.set_coeffs(P["coeff"], P["l1d"], P["a11"], P["a12"], P["albedo"])
        x = np.zeros(s.vec_shape)
        assert s.solve(P["b"], x).reason in (2, 3)
        c2 = P["coeff"].astype(np.float64) * (1.0 - 1e-9 * np.random.default_rng(5).random(P["coeff"].shape))
        s.set_coeffs(c2, P["l1d"], P["a11"], P["a12"], P["albedo"])
        v = np.random.default_rng(6).standard_normal(s.vec_shape)
        A = O.assemble_csr(lay, c2, P["l1d"], P["a11"], P["a12"], P["albedo"])
        y_ref = _par._ref_apply(dict(P, coeff=c2), lay, v)
        assert np.abs(s.apply(v) - y_ref).max() <= 1e-13 * np.abs(y_ref).max()
        for pc in (1, 2, 3):
            s.pc_apply(v, pc=pc, sweeps=2)
        x = np.zeros(s.vec_shape)
        assert s.solve(P["b"], x, rtol=1e-10, atol=1e-30, maxit=2000).reason == 2
        x_ref = spla.spsolve(A.tocsc(), P["b"].ravel()).reshape(x.shape)
        assert np.abs(x - x_ref).max() <= 1e-8 * np.abs(x_ref).max()
        info = s.solve(P["b"], x, rtol=1e-3, atol=1e-30, maxit=2000)   # warm start from the converged iterate
        assert info.reason in (2, 3) and np.abs(x - x_ref).max() <= 1e-8 * np.abs(x_ref).max()
        s.close()

    hostile(gpu, case)


# ---- exact scan (tsx_pcx.hip) ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nx,Ny,Nz,n1d", [(6, 8, 5, 0), (34, 6, 70, 3), (6, 4, 130, 0), (2, 2, 3, 0)])
def test_exact_scan_on_poisoned_memory(gpu, Nx, Ny, Nz, n1d):
    hostile(gpu, lambda mp: _par.test_exact_scan_preconditioner_is_checkerboard_gauss_seidel_to_rounding(gpu, Nx, Ny, Nz, n1d, 2))


def test_exact_scan_on_shared_blocks_on_poisoned_memory(gpu):
    hostile(gpu, lambda mp: _par.test_exact_scan_preconditioner_reads_shared_blocks_like_dense_ones(gpu, mp))


def test_failed_solve_retry_on_poisoned_memory(gpu):
    # (the body solves with a NaN initial guess and a NaN right-hand side on purpose: outputs may hold NaN in both runs)
    hostile(gpu, lambda mp: _par.test_failed_solve_is_retried_from_zero_with_the_conservative_solver(gpu, mp), finite=False)


# ---- flow kernel -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nx,Ny,Nz,field", [(64, 32, 20, "shared"), (128, 128, 12, "near"), (64, 64, 24, "own")])
def test_flow_kernel_on_poisoned_memory(gpu, Nx, Ny, Nz, field):
    hostile(gpu, lambda mp: _par.test_flow_kernel_is_bit_identical_to_launch_per_pass(gpu, mp, Nx, Ny, Nz, field))


def test_flow_kernel_self_neighbour_faces_on_poisoned_memory(gpu):
    # fat and lean bodies, faces through the mailbox
    hostile(gpu, lambda mp: _par.test_flow_kernel_with_self_neighbour_faces_is_bit_identical(gpu, mp, 64, 32, 20))


# ---- shared block storage --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,Nx,Ny,Nz,n1d", [("3_10", 10, 6, 5, 0), ("8_16", 8, 6, 5, 1)])
def test_shared_storage_on_poisoned_memory(gpu, solver, Nx, Ny, Nz, n1d):
    hostile(gpu, lambda mp: _par.test_shared_block_storage_is_lossless(gpu, mp, solver, Nx, Ny, Nz, n1d))


def test_sharing_from_lut_coordinates_on_poisoned_memory(gpu):
    hostile(gpu, lambda mp: _par.test_sharing_keyed_on_lut_coordinates_is_lossless(gpu, mp))


def test_sharing_taken_over_on_poisoned_memory(gpu):
    hostile(gpu, lambda mp: _par.test_sharing_structure_taken_over_from_the_previous_set_is_lossless(gpu, mp))


# ---- explicit solver -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nx,Ny,Nz,n1d,mixed", [(7, 5, 6, 2, 1), (16, 8, 20, 3, 0)])
def test_explicit_solver_on_poisoned_memory(gpu, Nx, Ny, Nz, n1d, mixed):
    hostile(gpu, lambda mp: _par.test_explicit_solver_shares_the_fixed_point_and_the_stop_rule_of_explicit_ediff(
        gpu, "3_10", Nx, Ny, Nz, n1d, mixed))


# ---- pipeline --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["3_10", "8_16"])
def test_solar_pipeline_on_poisoned_memory(gpu, solver):
    hostile(gpu, lambda mp: _pipe.test_solar_pipeline_matches_oracle(gpu, solver, 10.0, 60.0, 2, False))


@pytest.mark.parametrize("solver", ["3_10", "8_16"])
def test_thermal_pipeline_on_poisoned_memory(gpu, solver):
    hostile(gpu, lambda mp: _pipe.test_thermal_pipeline_matches_oracle(gpu, solver, "skin"))


@pytest.mark.parametrize("lsolar", [True, False])
def test_flux_divergence_on_poisoned_memory(gpu, lsolar):
    hostile(gpu, lambda mp: _pipe.test_absorption_by_flux_divergence_equals_coeff_divergence(gpu, lsolar))


# ---- seam ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [False, True])
def test_real32_seam_on_poisoned_memory(gpu, on_device):
    hostile(gpu, lambda mp: _seam.test_real32_vectors_cross_the_diffuse_seam_as_they_are(gpu, "3_10", on_device))


def test_direct_seam_on_poisoned_memory(gpu):
    hostile(gpu, lambda mp: _seam.test_direct_seam_equals_explicit_edir_and_setup_b(gpu, "3_10", 30.0, 20.0, 2))


# ---- LUT lookup ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,Nx,Ny,Nz", [("3_10", 21, 9, 12), ("8_16", 8, 5, 6)])
def test_device_lut_lookup_on_poisoned_memory(gpu, tmp_path, solver, Nx, Ny, Nz):
    hostile(gpu, lambda mp: _par.test_device_lut_lookup_bit_exact(gpu, solver, Nx, Ny, Nz, tmp_path))


# ---- multi-rank ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transport", ["host", "peer"])
def test_sharded_solve_on_poisoned_memory(gpu, transport):
    hostile(gpu, lambda mp: _mr.test_sharded_hip_solve_equals_global_oracle(gpu, 2, "3_10", 10, 13, transport))


def test_sharded_pipeline_over_peer_on_poisoned_memory(gpu):
    hostile(gpu, lambda mp: _mr.test_sharded_pipeline_equals_one_rank_pipeline(gpu, 4, 12, 10, 30.0, 55.0, 1, "peer"))


# ---- the detector itself ---------------------------------------------------------------------------------------------------------------
def test_pool_reports_a_damaged_red_zone_with_its_piece_and_offset(gpu, monkeypatch):
    """tsx_pool_debug_overrun writes a few bytes into the red zones of a piece of its own (never outside it): tsx_pool_check reports
    the piece's requested size and the offset of the first damaged byte from its end while it is live, tsx_dev_free finds the same
    when it is returned, a reset clears the finding.  Also inside the 256-byte rounding slack, where the write did no harm."""
    I64 = ctypes.c_int64
    monkeypatch.delenv("TSX_POOL_POISON", raising=False)
    st = (I64 * 4)()
    assert gpu.tsx_pool_debug_overrun(1000, 0, 3, st) != 0   # the mode is off: no zones to damage
    monkeypatch.setenv("TSX_POOL_POISON", POISON)
    assert pool_check(gpu, reset=1)[1] == 0
    for req, off, n in [(1000, 0, 3),            # just past the end
                        (1000, 20, 4),           # inside the rounding slack (1024 - 1000)
                        (1000, -1001, 1),        # the byte before the start: a poisoned index -1
                        (1000, -1008, 8),        # the element before the start
                        (4096, 4096 - 8, 8),     # the last bytes of the zone behind
                        (77, -77 - 4096, 1)]:    # the first byte of the zone in front
        assert gpu.tsx_pool_debug_overrun(req, off, n, st) == 0
        assert st[0] >= 1 and st[1] == 1 and st[2] == req and st[3] == off, (req, off, list(st))   # live
        assert pool_check(gpu, reset=1)[1:] == [1, req, off]     # found again when the piece was freed
        assert pool_check(gpu)[1] == 0
    for req, off, n in [(1000, 24 + 4096 - 2, 4), (1000, -1000 - 4097, 1), (1000, -3, 2)]:   # outside the zones: refused
        assert gpu.tsx_pool_debug_overrun(req, off, n, st) != 0
    monkeypatch.setenv("TSX_POOL", "0")   # straight to the driver: no zones, refused
    assert gpu.tsx_pool_debug_overrun(1000, 0, 3, st) != 0
    monkeypatch.delenv("TSX_POOL")
    assert pool_check(gpu)[1] == 0
