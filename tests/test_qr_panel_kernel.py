"""The QR panel factorization (qr_factor_hand: k_qr_panel_mw, its MFMA and
VALU helper applies, the k_geqr2 fallback, k_larft_diag and the blocked T
combine) through _core.qr_factor_hip, against LAPACK.

The reference is np.linalg.qr(A0, mode="raw"), LAPACK's dgeqrf, with T built
from its V and tau by a NumPy dlarft (forward, column-wise). The kernels
follow LAPACK's convention (beta = -sign(alpha) * norm, v_0 = 1), so R, V,
tau and T compare elementwise.

Checks on every case:
 a. backward error ||A0 - Q [R; 0]||_F / ||A0||_F, Q = I - V T V^T applied
    without forming Q;
 b. max |T + T^T - T^T (V^T V) T|, which is Q^T Q - I compressed to k x k
    and ties T to V;
 c. structure: T exactly zero below its diagonal, diag(T) zero or in [1, 2],
    all finite, the NaN pad rows of an odd lda = m + 3 and two sentinel
    columns past k unchanged bit for bit, and for a stacked [R; B] tile the
    block of V between R's diagonal and ts_split exactly zero;
 d. R, V, tau and T within 1e-10 of LAPACK's, each relative to that array's
    largest magnitude. This catches sign, scaling and indexing errors, which
    are O(1); it is not the precision check (V of a square matrix depends on
    conditioning: two correct Householder codes differ by 3e-14 at 1024).

Tolerance of a and b: the same quantity, by the same code, for LAPACK's own
factorization of the same input, times 8. A plain column-order Householder
stays within 2.3 x LAPACK on both measures at these shapes; the factor leaves
room for the kernel's tree reductions and MFMA summation order. The measures
are evaluated in long double where m * k * k <= 3e7 and in float64 above
(long double has no BLAS behind it).

impl="cpu" (the CPU chore's kernels) runs the small shapes and every edge
input without a GPU, which shows that the reference and the thresholds hold
independently of the hand kernels.

Worst kernel/LAPACK ratio per shape, impl="hand", measured on an MI355X over
every case of this file that uses the shape (every run prints them again
under pytest -s); the bound is 8:

    shape (m, k, ts_split)    a: backward   b: orthogonality
    (40, 40, 0)                  1.05          1.26
    (128, 128, 0)                1.00          0.79
    (200, 200, 0)                1.24          2.68
    (520, 200, 0)                1.46          0.80
    (1024, 1024, 0)              1.20          1.25
    (1152, 128, 0)               1.13          0.95
    (1153, 128, 0)               1.15          0.78
    (1280, 256, 0)               1.36          1.00
    (1300, 140, 0)               1.35          1.11
    (2304, 128, 0)               1.20          1.12
    (2305, 128, 0)               1.31          1.14
    (2400, 256, 0)               1.94          0.88
    (256, 128, 128)              0.88          1.02
    (384, 192, 192)              0.91          0.84
    (400, 200, 200)              1.15          1.33
    (512, 256, 256)              0.94          1.33
    (2048, 1024, 1024)           1.30          1.17
    (2176, 1088, 1088)           1.31          1.00

The rocSOLVER route stays below 1.33 and the CPU kernels below 3.15 (the
orthogonality of (400, 200, 200) with a zero diagonal).
"""
import functools

import numpy as np
import pytest

from parsec_amd import _core

GPU = pytest.mark.gpu

# (m, k, ts_split): the path each one takes is in the comment
SHAPES = [
    (40, 40, 0),          # partial last sub-panel
    (128, 128, 0),        # one full panel
    (200, 200, 0),        # second panel 72 wide, its last sub-panel 8 wide
    (520, 200, 0),        # tall, partial 256-row MFMA chunk
    (1024, 1024, 0),      # the benchmark's GEQRT
    (1152, 128, 0),       # last W=16 size
    (1153, 128, 0),       # first W=8 size
    (1280, 256, 0),       # W=8, then W=16
    (1300, 140, 0),       # W=8 twice; second panel 12 wide, sub-panels 8 + 4
    (2304, 128, 0),       # last W=8 size
    (2305, 128, 0),       # k_geqr2 fallback
    (2400, 256, 0),       # fallback + larfb_gemm, then W=8
    (256, 128, 128),      # stacked TSQRT tiles
    (384, 192, 192),
    (400, 200, 200),
    (512, 256, 256),
    (2048, 1024, 1024),   # the benchmark's TSQRT: rows == 1152 in every panel
    (2176, 1088, 1088),   # W=8 in the stacked row map
]
CPU_SHAPES = [s for s in SHAPES if s[0] <= 520]
ROCSOLVER_SHAPES = [(200, 200, 0), (1280, 256, 0), (512, 256, 256)]
CONFIG_SHAPES = [(40, 40, 0), (200, 200, 0), (520, 200, 0), (400, 200, 200),
                 (1300, 140, 0)]  # the last: every configuration at W=8 too
EDGE_SHAPES = [(200, 200, 0), (400, 200, 200)]
# (wgs, poolA, apply, lookahead)
CONFIGS = [
    (48, 15, "kernel", 1),  # the default
    (48, 15, "kernel", 0),
    (48, 15, "valu", 1),
    (48, 15, "gemm", 1),
    (2, 1, "kernel", 1),
    (16, 15, "kernel", 1),  # no pool B: pool A takes the trailing columns
    (20, 3, "kernel", 1),
]
FACTOR = 8.0
CONVENTION_TOL = 1e-10
LONGDOUBLE_MAX = 3e7


def _sid(s):
    return "x".join(str(v) for v in s)


def _impl_shape_params():
    out = []
    for s in SHAPES:
        out.append(pytest.param("hand", s, id=f"hand-{_sid(s)}", marks=GPU))
    for s in ROCSOLVER_SHAPES:
        out.append(pytest.param("rocsolver", s, id=f"rocsolver-{_sid(s)}",
                                marks=GPU))
    for s in CPU_SHAPES:
        out.append(pytest.param("cpu", s, id=f"cpu-{_sid(s)}"))
    return out


def _edge_params():
    out = []
    for s in EDGE_SHAPES:
        out.append(pytest.param("hand", s, id=f"hand-{_sid(s)}", marks=GPU))
        out.append(pytest.param("cpu", s, id=f"cpu-{_sid(s)}"))
    return out


# ------------------------------------------------------------------ inputs
def _make_input(shape, kind="dense"):
    m, k, ts = shape
    rng = np.random.default_rng(1000 + 7 * m + 3 * k + ts)
    A = rng.standard_normal((m, k))
    if ts:
        A[:ts] = np.triu(A[:ts])
    if kind == "triu":
        A = np.triu(A)
    elif kind == "mixed":      # triu in the first 20 columns, dense after
        A[:, :20] = np.triu(A)[:, :20]
    elif kind == "diag0":
        A[np.arange(k), np.arange(k)] = 0.0
    elif kind == "diagneg":
        A[np.arange(k), np.arange(k)] = -np.abs(np.diag(A))
    else:
        assert kind == "dense", kind
    A.setflags(write=False)
    return A


# --------------------------------------------------------------- reference
def _np_larft(V, tau):
    """dlarft, forward and column-wise: H_0 ... H_{k-1} = I - V T V^T."""
    k = len(tau)
    G = V.T @ V
    T = np.zeros((k, k))
    for i in range(k):
        T[i, i] = tau[i]
        if i:
            T[:i, i] = -tau[i] * (T[:i, :i] @ G[:i, i])
    return T


def _measures(A0, V, R, T):
    """(a, b) of the module docstring for one factorization."""
    m, k = A0.shape
    dt = np.longdouble if m * k * k <= LONGDOUBLE_MAX else np.float64
    A0, V, R, T = (x.astype(dt) for x in (A0, V, R, T))
    QR = -(V @ (T @ (V[:k].T @ R)))
    QR[:k] += R
    nrm = np.sqrt((A0 * A0).sum())
    a = np.sqrt(((A0 - QR) ** 2).sum()) / nrm if nrm else 0.0
    b = np.abs(T + T.T - T.T @ ((V.T @ V) @ T)).max()
    return float(a), float(b)


@functools.lru_cache(maxsize=None)
def _reference(shape, kind="dense"):
    """LAPACK's factorization of the input and its own measures, computed
    once per input and shared read-only."""
    m, k, ts = shape
    A0 = _make_input(shape, kind)
    h, tau = np.linalg.qr(A0, mode="raw")
    F = np.array(h.T)
    V = np.tril(F, -1)
    V[np.arange(k), np.arange(k)] = 1.0
    R = np.triu(F[:k])
    T = _np_larft(V, tau)
    a, b = _measures(A0, V, R, T)
    ref = dict(A0=A0, V=V, R=R, tau=tau, T=T, a=a, b=b)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


# ------------------------------------------------------------------ kernel
def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def _factor(A0, ts, impl, cfg=None):
    """Factor A0 in a buffer with lda = m + 3 (NaN pad rows) and two
    sentinel columns, assert what must hold of the buffer itself (check c),
    and return V, R, tau, T and the factored m x k block."""
    m, k = A0.shape
    lda = m + 3
    buf = np.full((lda, k + 2), np.nan, order="F")
    buf[:m, :k] = A0
    buf[:m, k] = 1234.5
    buf[:m, k + 1] = -np.arange(1, m + 1)
    before = buf.copy(order="F")
    flat = buf.ravel(order="F")
    assert np.shares_memory(flat, buf)  # factored in place, through a view
    kw = {}
    if cfg is not None:
        kw = dict(wgs=cfg[0], poolA=cfg[1], apply=cfg[2], lookahead=cfg[3])
    T = _core.qr_factor_hip(flat, m, k, lda, ts, impl, **kw)
    F = buf[:m, :k]
    assert T.shape == (k, k)
    assert np.all(np.isfinite(F)), "non-finite factor"
    assert np.all(np.isfinite(T)), "non-finite T"
    assert np.array_equal(_bits(buf[m:]), _bits(before[m:])), "pad rows"
    assert np.array_equal(_bits(buf[:, k:]), _bits(before[:, k:])), \
        "sentinel columns"
    assert np.all(np.tril(T, -1) == 0.0), "T below its diagonal"
    tau = np.diag(T).copy()
    assert np.all((tau == 0.0) | ((tau >= 1.0) & (tau <= 2.0))), "tau range"
    if ts:
        assert np.all(np.tril(A0[:ts], -1) == 0.0)
        assert np.all(np.tril(F[:ts], -1) == 0.0), "V inside R's zero block"
    V = np.tril(F, -1)
    V[np.arange(k), np.arange(k)] = 1.0
    R = np.triu(F[:k])
    return dict(V=V, R=R, tau=tau, T=T, F=F.copy())


def _check(what, shape, impl, kind="dense", cfg=None):
    """Checks a to d of one factorization against the shared reference."""
    ref = _reference(shape, kind)
    got = _factor(ref["A0"], shape[2], impl, cfg)
    a, b = _measures(ref["A0"], got["V"], got["R"], got["T"])
    ra = a / ref["a"] if ref["a"] else (0.0 if a == 0 else np.inf)
    rb = b / ref["b"] if ref["b"] else (0.0 if b == 0 else np.inf)
    print(f"{what}: backward {a:.3e} (lapack {ref['a']:.3e}, x{ra:.2f}), "
          f"orth {b:.3e} (lapack {ref['b']:.3e}, x{rb:.2f})")
    for name in ("R", "V", "tau", "T"):
        scale = np.abs(ref[name]).max()
        d = np.abs(got[name] - ref[name]).max()
        print(f"  {name}: max diff to LAPACK {d:.3e}, max |{name}| {scale:.3e}")
        assert d <= CONVENTION_TOL * scale, f"{what}: {name} vs LAPACK"
    assert a <= FACTOR * ref["a"], f"{what}: backward error x{ra:.2f} LAPACK"
    assert b <= FACTOR * ref["b"], f"{what}: orthogonality x{rb:.2f} LAPACK"
    return got


# ------------------------------------------------------------------- tests
@pytest.mark.parametrize("impl,shape", _impl_shape_params())
def test_qr_factor_vs_lapack(impl, shape):
    """Every shape with the default tunables (none overridden)."""
    _check(f"{impl} {_sid(shape)}", shape, impl)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("shape", CONFIG_SHAPES, ids=_sid)
def test_qr_factor_configs(shape, cfg):
    """Apply modes, look-ahead off, and pool splits down to one helper."""
    _check(f"hand {_sid(shape)} cfg={cfg}", shape, "hand", cfg=cfg)


@pytest.mark.parametrize("impl,shape", _edge_params())
def test_qr_upper_triangular_input(impl, shape):
    """Nothing to annihilate: every tau is 0, T is zero and the matrix comes
    back bit for bit."""
    A0 = _make_input(shape, "triu")
    got = _factor(A0, shape[2], impl)
    assert np.array_equal(_bits(got["F"]), _bits(A0))
    assert np.all(got["T"] == 0.0)


@pytest.mark.parametrize("kind", ["mixed", "diag0", "diagneg"])
@pytest.mark.parametrize("impl,shape", _edge_params())
def test_qr_edge_inputs(impl, shape, kind):
    """mixed: tau = 0 and tau != 0 inside one sub-panel (columns 16..31), so
    the norm carried along with the previous column's update matters; diag0:
    alpha = +0.0 takes the positive sign; diagneg: every beta positive."""
    got = _check(f"{impl} {_sid(shape)} {kind}", shape, impl, kind=kind)
    if kind == "mixed":
        assert np.all(got["tau"][:20] == 0.0)
        assert np.all(got["tau"][20:-1] != 0.0)
    if kind == "diagneg":
        assert got["R"][0, 0] > 0


@pytest.mark.parametrize("exp", [300, -300])
@pytest.mark.parametrize("impl,shape", _edge_params())
def test_qr_power_of_two_scaling(impl, shape, exp):
    """Scaling the input by a power of two scales R exactly and leaves V,
    tau and T bit-identical while nothing overflows: the kernels do not
    rescale as dlarfg does, so this is as far as the exponent goes."""
    A0 = _make_input(shape)
    s = 2.0 ** exp
    base = _factor(A0, shape[2], impl)
    got = _factor(A0 * s, shape[2], impl)
    assert np.array_equal(_bits(got["R"]), _bits(base["R"] * s)), "R"
    for name in ("V", "tau", "T"):
        assert np.array_equal(_bits(got[name]), _bits(base[name])), name


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1024, 1024, 0), (2048, 1024, 1024)],
                         ids=_sid)
def test_qr_factor_deterministic(shape):
    """Each column has a fixed owner and reflectors apply in publication
    order, so three runs on one input agree bit for bit; a difference is a
    race."""
    A0 = _reference(shape)["A0"]
    runs = [_factor(A0, shape[2], "hand") for _ in range(3)]
    for r in runs[1:]:
        assert np.array_equal(_bits(r["F"]), _bits(runs[0]["F"])), "A"
        assert np.array_equal(_bits(r["T"]), _bits(runs[0]["T"])), "T"


def test_qr_factor_rejects_bad_arguments():
    A = np.zeros(8 * 4)
    for args, kw in [((A, 8, 4, 7), {}),                 # lda < m
                     ((A, 4, 8), {}),                    # m < k
                     ((A, 9, 4), {}),                    # buffer too small
                     ((A, 8, 4), dict(impl="magma")),
                     ((A, 8, 4), dict(apply="mfma")),
                     ((A, 8, 4), dict(wgs=49)),
                     ((A, 8, 4), dict(ts_split=3)),
                     ((A.reshape(8, 4), 8, 4), {})]:
        with pytest.raises(ValueError):
            _core.qr_factor_hip(*args, **kw)
