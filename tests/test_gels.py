"""insert_gels (Householder least squares / solve, the dgels analog): the
right-hand side rides through the tile QR of A and one backward sweep with R
finishes. Checked against LAPACK doing the same algorithm.

Inputs and the solve step live in _gels_worker.py, which is also the
subprocess worker of the cases that need a process of their own."""
import os
import subprocess
import sys

import numpy as np
import pytest

import parsec_amd as pm

import _gels_worker as gw

EPS = np.finfo(np.float64).eps
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                      "_gels_worker.py")


def _solve_upper(R, Y):
    try:
        from scipy.linalg import solve_triangular
        return solve_triangular(R, Y)
    except ImportError:
        return np.linalg.solve(R, Y)


_refs = {}


def _reference(case):
    """Input and LAPACK's solution by the same algorithm, computed once per
    case and left unchanged."""
    if case not in _refs:
        A0, B0 = gw.make_input(case)
        Q, R = np.linalg.qr(A0)
        X = _solve_upper(R, Q.T @ B0)
        for a in (A0, B0, X):
            a.setflags(write=False)
        _refs[case] = (A0, B0, X)
    return _refs[case]


def _gram_defect(A0, R):
    G = A0.T @ A0
    return np.linalg.norm(G - R.T @ R) / np.linalg.norm(G)


def _check_r_against_lapack(what, A0, R):
    """The helper of test_qr.py, for an m x n input: tile QR fixes R up to
    row signs, so |R| compares elementwise, and the Gram defect
    ||A0^T A0 - R^T R||_F / ||A0^T A0||_F may be at most 8 times what the same
    code gives for LAPACK's R.

    Bound on |R|: both are exact factors of matrices A0 + dA, and to first
    order ||dR||_F <= sqrt(2) cond(A0) ||R||_2 ||dA||_F / ||A0||_2 (Stewart's
    bound for the R factor). With ||dA||_F <= m eps ||A0||_2 for each of the
    two factorizations the difference is at most
    2 sqrt(2) m eps cond(A0) ||R||_2.

    test_qr.py has n where this has m, the number of rows: the same for its
    square input, and for tall input the growth factor of Householder QR's
    backward error goes with the column length. That makes the bound looser
    by M / N than a copy with n would be. It is loose in any case: at
    cond(A0) = 1e10 it is about 1.6e-3, and there the Gram defect is what
    constrains R."""
    m = A0.shape[0]
    Rl = np.linalg.qr(A0, mode="r")
    sv = np.linalg.svd(A0, compute_uv=False)
    bound = 2 * np.sqrt(2) * m * EPS * (sv[0] / sv[-1]) * sv[0]
    diff = np.abs(np.abs(R) - np.abs(Rl)).max()
    got, ref = _gram_defect(A0, R), _gram_defect(A0, Rl)
    print(f"{what}: max ||R|-|R_lapack|| = {diff:.3e} (bound {bound:.3e}, "
          f"cond {sv[0] / sv[-1]:.3e}); Gram defect {got:.3e} "
          f"(lapack {ref:.3e}, x{got / ref:.2f})")
    assert np.all(np.isfinite(R))
    assert diff <= bound, what
    assert got <= 8 * ref, what


def _measure(A0, B0, X):
    """Square A: the normwise backward error eta(X) of A X = B. Tall A: the
    normal-equations residual rho(X), which vanishes at the least-squares
    solution."""
    na, res = np.linalg.norm(A0), B0 - A0 @ X
    scale = na * np.linalg.norm(X) + np.linalg.norm(B0)
    if A0.shape[0] == A0.shape[1]:
        return np.linalg.norm(res) / scale
    return np.linalg.norm(A0.T @ res) / (na * scale)


def _check(what, case, Af, Bf):
    """Af, Bf: A and B after insert_gels.

    X (rows [0, N) of B) is accepted when everything is finite and its
    measure is at most 8 times the measure of LAPACK's X, floored at eps (no
    computed solution is expected below unit roundoff); R (A's upper tiles)
    by _check_r_against_lapack.

    Tall A: the column norms of rows [N, M) of B must equal the residual
    norms ||b - A0 x_ref|| per column. In exact arithmetic those rows are
    Q2^T b with [Q1 Q2] the full Q, and ||Q2^T b|| = ||b - A0 x||. The
    computed rows are exact for A0 + dA, b + db with ||dA|| <= g ||A0||,
    ||db|| <= g ||b||, g = sqrt(M) eps (Householder QR is backward stable; g
    is its rounding growth over columns of length M). To first order the
    residual r of a least-squares problem moves by
    dr = P (db - dA x) - pinv(A0)^T dA^T r, P the projector onto range(A0)'s
    complement, so | ||r~|| - ||r|| | <= g (||b|| + ||A0|| ||x||) +
    g cond(A0) ||r||. The reference's ||b - A0 x_ref|| is as good to first
    order (an error of x_ref inside range(A0) is orthogonal to r), which
    doubles it: relative tolerance
    2 sqrt(M) eps (cond(A0) + (||A0||_2 ||x|| + ||b||) / ||r||)."""
    A0, B0, Xref = _reference(case)
    m, n = A0.shape
    assert np.all(np.isfinite(Bf)), what
    X = Bf[:n]
    got, ref = _measure(A0, B0, X), _measure(A0, B0, Xref)
    print(f"{what}: measure {got:.3e} (lapack {ref:.3e}), "
          f"max |X - X_lapack| / max |X_lapack| = "
          f"{np.abs(X - Xref).max() / np.abs(Xref).max():.3e}")
    assert got <= 8 * max(ref, EPS), what
    _check_r_against_lapack(what, A0, np.triu(Af[:n]))
    if m > n:
        sv = np.linalg.svd(A0, compute_uv=False)
        r = np.linalg.norm(B0 - A0 @ Xref, axis=0)
        rest = np.linalg.norm(Bf[n:], axis=0)
        tol = 2 * np.sqrt(m) * EPS * (
            sv[0] / sv[-1] + (sv[0] * np.linalg.norm(Xref, axis=0) +
                              np.linalg.norm(B0, axis=0)) / r)
        rel = np.abs(rest - r) / r
        print(f"{what}: residual norms, max rel diff {rel.max():.3e} "
              f"(min tolerance {tol.min():.3e})")
        assert np.all(rel <= tol), what


def _cpu_ctx():
    ctx = pm.Context(nworkers=2, rank=0, world=1, gpu=-2)
    assert not ctx.has_gpu
    return ctx


def _run_worker(tmp_path, cases, env_extra, extra_args=(), name="out.npz"):
    out = str(tmp_path / name)
    env = dict(os.environ)
    env.update(env_extra)
    r = subprocess.run([sys.executable, WORKER, out, ",".join(cases),
                        *extra_args], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "GELS_WORKER_OK" in r.stdout, \
        r.stdout + r.stderr
    return np.load(out)


def _case_tiles(z, case):
    pre = case + ":"
    return {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}


@pytest.mark.parametrize("case", ["tall_cpu", "square_cpu"])
def test_gels_cpu(case):
    """Tall 320 x 192 and square 256 x 256, nb = 64, nrhs = 96: one full and
    one 32-wide column tile of B."""
    ctx = _cpu_ctx()
    Af, Bf = gw.assemble(case, gw.solve_tiles(ctx, case))
    _check(f"cpu {case}", case, Af, Bf)
    del ctx


def test_gels_cpu_ill_conditioned():
    """A0 = U diag(logspace(0, -10, 256)) V^T: cond(A0) = 1e10, far outside
    the cond <~ 1e7 envelope of insert_gels_bcgs. Householder QR is backward
    stable whatever the conditioning, so the backward error stays at
    LAPACK's."""
    ctx = _cpu_ctx()
    Af, Bf = gw.assemble("illcond", gw.solve_tiles(ctx, "illcond"))
    _check("cpu cond 1e10", "illcond", Af, Bf)
    del ctx


def test_gels_cpu_needs_pivoting():
    """Gaussian with its leading 64 x 64 block zero: LU without pivoting
    meets a zero pivot in its first tile (insert_gesv_nopiv would abort the
    process on it), QR needs no pivoting."""
    ctx = _cpu_ctx()
    Af, Bf = gw.assemble("zeroblock", gw.solve_tiles(ctx, "zeroblock"))
    _check("cpu zero leading block", "zeroblock", Af, Bf)
    del ctx


def test_gels_cpu_binary_tree(tmp_path):
    """The tall case with qr_tree=binary, which is read when the DAG is
    built; in a process of its own so the setting does not leak."""
    z = _run_worker(tmp_path, ["tall_cpu"], {"GELS_TREE": "binary"})
    Af, Bf = gw.assemble("tall_cpu", _case_tiles(z, "tall_cpu"))
    _check("cpu binary tree", "tall_cpu", Af, Bf)


def test_gels_world2(tmp_path):
    """The tall case on a 2 x 1 grid of two processes over the TCP engine."""
    from conftest import port_base
    port = str(port_base(23))
    procs = []
    for r in range(2):
        env = dict(os.environ)
        env.update(RANK=str(r), WORLD_SIZE="2", PORT=port)
        procs.append(subprocess.Popen(
            [sys.executable, WORKER, str(tmp_path / f"rank{r}.npz"),
             "tall_cpu"], env=env, stdout=subprocess.PIPE,
            stderr=subprocess.STDOUT))
    for pr in procs:
        o, _ = pr.communicate(timeout=180)
        assert pr.returncode == 0 and b"GELS_WORKER_OK" in o, o.decode()
    tiles = {}
    for r in range(2):
        tiles.update(_case_tiles(np.load(tmp_path / f"rank{r}.npz"),
                                 "tall_cpu"))
    Af, Bf = gw.assemble("tall_cpu", tiles)
    _check("cpu 2 x 1 grid", "tall_cpu", Af, Bf)


def test_geqrf_unchanged_by_gels():
    """insert_geqrf is the sweep of insert_gels without B: on the 576/192
    input of test_qr.py both leave bit-identical R."""
    ctx = _cpu_ctx()
    Aq, _ = gw.assemble("qr_dag", gw.solve_tiles(ctx, "qr_dag",
                                                 factor_only=True))
    Ag, _ = gw.assemble("qr_dag", gw.solve_tiles(ctx, "qr_dag"))
    assert np.array_equal(np.triu(Aq), np.triu(Ag))
    _check_r_against_lapack("geqrf", gw.make_input("qr_dag")[0], np.triu(Aq))
    del ctx


# The GPU cases run in the worker with a small device pool: a context takes
# 85% of the free device memory by default, and the driver hands a pool of
# that size back only some time after its process has gone, time in which the
# GPU tests that follow would find the device nearly full.
GPU_ENV = {"GELS_GPU": "1", "PARSEC_MCA_gpu_mem_limit_mb": "2048"}


@pytest.mark.gpu
def test_gels_gpu(tmp_path):
    """Default chores, nb = 192 (no multiple of 128): 768 x 576 and
    576 x 576 with nrhs = 256, one full and one 64-wide column tile of B."""
    z = _run_worker(tmp_path, ["tall_gpu", "square_gpu"], GPU_ENV)
    assert int(z["gpu_tasks"]) > 0
    assert str(z["chore_gemm_nn"]) == os.environ.get(
        "PARSEC_MCA_chore_gemm_nn", "rocblas")
    for case in ("tall_gpu", "square_gpu"):
        Af, Bf = gw.assemble(case, _case_tiles(z, case))
        _check(f"gpu {case}", case, Af, Bf)


@pytest.mark.gpu
def test_gels_gpu_hip_gemm_nn_chore(tmp_path):
    """PARSEC_MCA_chore_gemm_nn=hip, in a process of its own because chores
    are chosen once per process: the two GPU problems, and insert_gesv_nopiv
    on the diagonally dominant problem of
    test_lu.py::test_gesv_nopiv_vs_numpy with its 1e-10 criterion, where the
    hand kernel meets tiles 64 and 32 wide, below one block."""
    z = _run_worker(tmp_path, ["tall_gpu", "square_gpu"],
                    {**GPU_ENV, "PARSEC_MCA_chore_gemm_nn": "hip"},
                    extra_args=("gesv",))
    assert int(z["gpu_tasks"]) > 0
    # the setting reached the chore selection of the process that ran the DAGs
    assert str(z["chore_gemm_nn"]) == "hip"
    for case in ("tall_gpu", "square_gpu"):
        Af, Bf = gw.assemble(case, _case_tiles(z, case))
        _check(f"gpu hip gemm_nn {case}", case, Af, Bf)
    err = float(z["gesv_err"])
    print(f"gesv_nopiv with the hand gemm_nn: rel err {err:.3e}")
    assert err < 1e-10, err
