"""The exact fp64 red-black scan preconditioner of 8_16 (tsx_pcx.hip, tsx_k_pcx16_rb): with fp64 directions and the operator's own
blocks (fp32_directions = 0, pc_coeff_fp16 = 0 -- the reference's default `ireals`), TSX_PC_REDBLACK on 8_16 is checkerboard
Gauss-Seidel over exact column-block solves, as it is on 3_10.  Before it existed, 8_16 fell back to zebra rows on this path (and on
the retry after every failed solve)."""
import numpy as np
import pytest

import test_gpu_parity as _par
import test_gpu_pool_hostile as _hostile
from oracle import oracle as O
from tenstream_amd import DiffuseSolver, lut, synthetic

pytestmark = pytest.mark.gpu


def _owners(lay, n):
    """owner column (i, j) of every unknown in the reference numbering (as _column_block_matrix assigns them)"""
    D, L, Nx, Ny, Nz = lay.D, lay.Nz + 1, lay.xm, lay.ym, lay.Nz
    idx = np.arange(n)
    d, k = idx % D, (idx // D) % L
    i, j = (idx // (D * L)) % Nx, idx // (D * L * Nx)
    oi, oj = i.copy(), j.copy()
    qx, qy = d - lay.ntop, d - lay.ntop - lay.nside
    mx = (qx >= 0) & (qx < lay.nside) & (qx % 2 == 1) & (k < Nz)
    my = (qy >= 0) & (qy < lay.nside) & (qy % 2 == 1) & (k < Nz)
    oi[mx] = (i[mx] - 1) % Nx
    oj[my] = (j[my] - 1) % Ny
    return oi, oj


def _checkerboard_gs(P, lay, v, sweeps, faces=False):
    """sparse model: sweeps + 1 passes, colour (i + j) & 1 alternately, exact column-block solves with the other colour's latest
    values on the right-hand side.  faces: the couplings across the domain's edges are dropped (nothing wraps)"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla

    M, A = _par._column_block_matrix(P, lay)
    oi, oj = _owners(lay, A.shape[0])
    colour = (oi + oj) % 2
    Noff = (A - M.tocsr()).tocoo()
    if faces:
        keep = (np.abs(oi[Noff.row] - oi[Noff.col]) <= 1) & (np.abs(oj[Noff.row] - oj[Noff.col]) <= 1)
        Noff = sp.csr_matrix((Noff.data[keep], (Noff.row[keep], Noff.col[keep])), shape=A.shape)
    else:
        Noff = Noff.tocsr()
    lu = spla.splu(M.tocsc(), permc_spec="NATURAL")
    x = np.zeros(v.size)
    for p_ in range(sweeps + 1):
        rhs = v.ravel() - (Noff @ x if p_ > 0 else 0.0)
        mk = colour == (p_ % 2)
        x[mk] = lu.solve(rhs)[mk]
    return x


# 1-D layers, odd Nz, 16 / 32 / 64 segments per column (Nz <= 64 / 128 / 256), a minimal 2 x 2 grid, a long row
SHAPES = [(8, 6, 6, 1), (6, 4, 5, 0), (4, 6, 7, 2), (6, 4, 70, 3), (4, 4, 130, 0), (2, 2, 3, 0), (34, 4, 4, 0)]


@pytest.mark.parametrize("Nx,Ny,Nz,n1d", SHAPES)
@pytest.mark.parametrize("sweeps", [1, 2, 5])
def test_exact_scan_8_16_is_checkerboard_gauss_seidel_to_rounding(gpu, Nx, Ny, Nz, n1d, sweeps):
    """M^-1 v with fp64 directions equals the sparse-direct checkerboard model to rounding (zebra rows: an O(1) difference)"""
    P = synthetic.make_problem("8_16", Nx=Nx, Ny=Ny, Nz=Nz, n1d=n1d)
    lay = O.layout("8_16", Nz, Nx, Ny)
    v = np.random.default_rng(4).standard_normal(P["b"].shape)
    x = _checkerboard_gs(P, lay, v, sweeps)
    s = DiffuseSolver("8_16", Nz, Nx, Ny)
    s.set_coeffs(P["coeff"], P["l1d"], P["a11"], P["a12"], P["albedo"])
    z = s.pc_apply(v, pc=3, sweeps=sweeps, mixed=False)
    assert np.abs(z.ravel() - x).max() <= 1e-11 * np.abs(x).max()
    s.close()


@pytest.mark.parametrize("Nx,Ny,Nz,n1d", [(8, 6, 6, 1), (6, 4, 70, 3), (2, 2, 3, 0)])
def test_exact_scan_8_16_solve_reaches_the_sparse_direct_solution(gpu, Nx, Ny, Nz, n1d):
    """nothing reduced anywhere: fp64 directions on the exact blocks reach the sparse-direct solution; red-black ran, not zebra"""
    import scipy.sparse.linalg as spla

    P = synthetic.make_problem("8_16", Nx=Nx, Ny=Ny, Nz=Nz, n1d=n1d)
    lay = O.layout("8_16", Nz, Nx, Ny)
    A = O.assemble_csr(lay, P["coeff"].astype(np.float64), P["l1d"], P["a11"], P["a12"], P["albedo"])
    s = DiffuseSolver("8_16", Nz, Nx, Ny)
    s.set_coeffs(P["coeff"], P["l1d"], P["a11"], P["a12"], P["albedo"])
    xs = np.zeros(s.vec_shape)
    info = s.solve(P["b"], xs, rtol=1e-12, atol=1e-30, pc=3, fp32_directions=0, pc_coeff_fp16=0)
    assert info.reason == 2
    x_ref = spla.spsolve(A.tocsc(), P["b"].ravel()).reshape(P["b"].shape)
    assert np.abs(xs - x_ref).max() <= 1e-9 * np.abs(x_ref).max()
    assert s.pc_info()[0] == 3
    s.close()


def test_exact_scan_8_16_reads_shared_blocks_like_dense_ones(gpu, monkeypatch):
    """LUT path: the passes read the entry-major shared blocks through the per-cell index -- the same z, bit for bit, as with every
    cell's block in dense planes (TSX_DEDUP=0)"""
    Nx, Ny, Nz = 12, 8, 9
    kabs, ksca, g = synthetic.cloud_field(Nx, Ny, Nz, seed=3)
    kabs, ksca, g = synthetic.delta_scale(kabs, ksca, g)
    dz = np.full((Ny, Nx, Nz), 50.0)
    l1d = np.zeros(Nz, dtype=np.uint8)
    l1d[0] = 1
    a11, a12 = 0.6 + 0.0 * kabs, 0.1 + 0.0 * kabs
    alb = np.full((Ny, Nx), 0.2)
    v = np.random.default_rng(1).standard_normal((Ny, Nx, Nz + 1, 16))
    out = {}
    for dd in ("1", "0"):
        monkeypatch.setenv("TSX_DEDUP", dd)
        s = DiffuseSolver("8_16", Nz, Nx, Ny)
        s.set_lut_diffuse(lut.synthetic_diffuse_table("8_16"), lut.diffuse_axes("8_16"))
        s.set_optprop(kabs, ksca, g, dz, 100.0, l1d, a11, a12, alb)
        out[dd] = s.pc_apply(v, pc=3, sweeps=3, mixed=False)
        if dd == "1":
            assert s.dedup_info()[0]
        s.close()
    assert np.isfinite(out["1"]).all()
    assert np.array_equal(out["1"], out["0"])


def test_exact_scan_8_16_on_fp64_planes(gpu):
    """blocks that fp32 cannot hold are kept as fp64 planes and read as they are: the model on those blocks, to rounding"""
    Nx, Ny, Nz = 6, 4, 5
    P = synthetic.make_problem("8_16", Nx=Nx, Ny=Ny, Nz=Nz, n1d=1)
    rng = np.random.default_rng(3)
    c = P["coeff"].astype(np.float64) * (1.0 - 1e-9 * rng.random(P["coeff"].shape))
    P = dict(P, coeff=c)
    lay = O.layout("8_16", Nz, Nx, Ny)
    v = rng.standard_normal(P["b"].shape)
    x = _checkerboard_gs(P, lay, v, 2)
    s = DiffuseSolver("8_16", Nz, Nx, Ny)
    s.set_coeffs(c, P["l1d"], P["a11"], P["a12"], P["albedo"])
    z = s.pc_apply(v, pc=3, sweeps=2, mixed=False)
    assert np.abs(z.ravel() - x).max() <= 1e-11 * np.abs(x).max()
    s.close()


@pytest.mark.parametrize("Nx,Ny,Nz,n1d", [(6, 4, 5, 1), (4, 5, 7, 0)])
def test_exact_scan_8_16_drops_the_couplings_across_rank_faces(gpu, Nx, Ny, Nz, n1d):
    """force_halo: the faces go through the halo path and do not wrap; the passes drop the couplings across them (block Jacobi over
    ranks, as the reference's PCBJACOBI) -- an odd number of rows is eligible there"""
    P = synthetic.make_problem("8_16", Nx=Nx, Ny=Ny, Nz=Nz, n1d=n1d)
    lay = O.layout("8_16", Nz, Nx, Ny)
    v = np.random.default_rng(7).standard_normal(P["b"].shape)
    x = _checkerboard_gs(P, lay, v, 3, faces=True)
    s = DiffuseSolver("8_16", Nz, Nx, Ny, force_halo=1)
    s.set_coeffs(P["coeff"], P["l1d"], P["a11"], P["a12"], P["albedo"])
    z = s.pc_apply(v, pc=3, sweeps=3, mixed=False)
    assert np.abs(z.ravel() - x).max() <= 1e-11 * np.abs(x).max()
    s.close()


def test_failed_8_16_solve_is_retried_on_the_exact_scan(gpu):
    """a NaN in the initial guess fails the first attempt; the retry (exact blocks, fp64 directions, red-black scan) converges to
    the sparse-direct solution"""
    import scipy.sparse.linalg as spla

    P = synthetic.make_problem("8_16", Nx=8, Ny=6, Nz=6, n1d=1)
    lay = O.layout("8_16", 6, 8, 6)
    A = O.assemble_csr(lay, P["coeff"].astype(np.float64), P["l1d"], P["a11"], P["a12"], P["albedo"])
    x_ref = spla.spsolve(A.tocsc(), P["b"].ravel()).reshape(P["b"].shape)
    s = DiffuseSolver("8_16", 6, 8, 6)
    s.set_coeffs(P["coeff"], P["l1d"], P["a11"], P["a12"], P["albedo"])
    x = np.zeros(s.vec_shape)
    x[2, 3, 1, 5] = np.nan
    info = s.solve(P["b"], x, rtol=1e-10, atol=1e-30)
    assert info.reason == 2 and np.isfinite(x).all()
    assert np.abs(x - x_ref).max() <= 1e-8 * np.abs(x_ref).max()
    assert s.pc_info()[0] == 3
    s.close()


def test_exact_scan_8_16_full_size_default_tolerances(gpu):
    """256 x 256 x 64 (config 5's domain), everything fp64, the reference's default tolerances: a few iterations (zebra rows: 37)"""
    Nx, Ny, Nz, dx, dz, albedo = 256, 256, 64, 100.0, 50.0, 0.1
    kabs, ksca, g = synthetic.cloud_field(Nx, Ny, Nz)
    kabs, ksca, g = synthetic.delta_scale(kabs, ksca, g)
    b = synthetic.solar_source("8_16", kabs, ksca, g, dz, dx, np.full((Ny, Nx), albedo))
    s = DiffuseSolver("8_16", Nz, Nx, Ny)
    s.set_lut_diffuse(lut.synthetic_diffuse_table("8_16"), lut.diffuse_axes("8_16"))
    zero = np.zeros((Ny, Nx, Nz))
    s.set_optprop(kabs, ksca, g, np.full((Ny, Nx, Nz), dz), dx, np.zeros(Nz, dtype=np.uint8), zero, zero,
                  np.full((Ny, Nx), albedo))
    x = np.zeros(s.vec_shape)
    info = s.solve(b, x, fp32_directions=0, pc_coeff_fp16=0)
    assert info.reason == 2, info
    assert info.niter <= 8, info
    assert s.pc_info()[0] == 3
    assert np.isfinite(x).all()
    s.close()


# ---- hostile memory (TSX_POOL_POISON, tsx_pool.hip): the records and the colour-split copies rely on nothing they never wrote ----------
@pytest.mark.parametrize("Nx,Ny,Nz,n1d", [(8, 6, 6, 1), (6, 4, 70, 3), (4, 4, 130, 0), (2, 2, 3, 0)])
def test_exact_scan_8_16_on_poisoned_memory(gpu, Nx, Ny, Nz, n1d):
    _hostile.hostile(gpu, lambda mp: test_exact_scan_8_16_is_checkerboard_gauss_seidel_to_rounding(gpu, Nx, Ny, Nz, n1d, 2))


def test_exact_scan_8_16_solve_on_poisoned_memory(gpu):
    _hostile.hostile(gpu, lambda mp: test_exact_scan_8_16_solve_reaches_the_sparse_direct_solution(gpu, 8, 6, 6, 1))


def test_exact_scan_8_16_shared_blocks_on_poisoned_memory(gpu):
    _hostile.hostile(gpu, lambda mp: test_exact_scan_8_16_reads_shared_blocks_like_dense_ones(gpu, mp))


def test_exact_scan_8_16_fp64_planes_on_poisoned_memory(gpu):
    _hostile.hostile(gpu, lambda mp: test_exact_scan_8_16_on_fp64_planes(gpu))
