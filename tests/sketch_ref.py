"""NumPy statements of what the device-resident sketching path computes (csrc/aqc_sketch.hip, csrc/aqc_philox.h):
the (seed, stream, iteration, lane, plane) -> Philox counter rule of the draws, Box-Muller on those uniforms, CholeskyQR2,
the three generators built from them and the ADAM walk of optimizer._adam on a fixed sequence of sketches."""
import numpy as np

SKETCH_RAND, SKETCH_ALT, SKETCH_EIGEN = 0, 1, 2      # AQC_SKETCH_* of include/aqc_hip.h; also the Philox stream of the kind
QR_RANK_DEFICIENT = 1                                # AQC_QR_RANK_DEFICIENT


def plane_uniforms(seed: int, stream: int, iteration: int, lane: int, plane: int, count: int) -> np.ndarray:
    """``count`` uniform doubles of one plane.  key = [seed, stream], counter = [0, iteration, lane, plane]: NumPy advances the
    counter before its first block, so element e is word e % 4 of the block of counter [1 + e // 4, iteration, lane, plane]."""
    bitgen = np.random.Philox(key=np.array([seed, stream], dtype=np.uint64), counter=np.array([0, iteration, lane, plane], dtype=np.uint64))
    return np.random.Generator(bitgen).random(count)


def box_muller(u1: np.ndarray, u2: np.ndarray) -> np.ndarray:
    """Standard normals from two planes of uniforms: sqrt(-2 log(1 - u1)) cos(2 pi u2); 1 - u1 is exact and never 0."""
    return np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(6.283185307179586 * u2)


def omega(kind: int, seed: int, iteration: int, lane: int, d: int, k: int) -> np.ndarray:
    """The (d, k) complex draw of lane ``lane`` for sketch number ``iteration``."""
    u = [plane_uniforms(seed, kind, iteration, lane, p, d * k) for p in range(2 if kind == SKETCH_RAND else 4)]
    if kind == SKETCH_RAND:
        return (u[0] + 1j * u[1]).reshape(d, k)
    return (box_muller(u[0], u[1]) + 1j * box_muller(u[2], u[3])).reshape(d, k)


def cholesky_qr2(a: np.ndarray) -> np.ndarray:
    """Q of A = Q R by two passes of (G = A^H A = L L^H, A <- A L^-H)."""
    q = np.array(a, dtype=np.complex128)
    for _ in range(2):
        low = np.linalg.cholesky(np.conj(q.T) @ q)
        q = np.linalg.solve(low, np.conj(q.T)).conj().T
    return q


PIVOT_REL = 1e-10      # kPivotRel of csrc/aqc_sketch.hip
ORTH_TOL = 1e-4        # kOrthTol: the largest entry of G2 - I a lane may show in the second pass


def cholesky_qr2_rule(a: np.ndarray, pivot_rel: float = PIVOT_REL, abs_floor: float = 0.0, orth_tol: float = ORTH_TOL) -> tuple:
    """The device's QR with its status rule, (q, status): two passes of Gram matrix, right-looking Cholesky and triangular solve.
    A pivot that is not finite, not above ``pivot_rel`` times its diagonal entry of that pass's Gram matrix or not above
    ``abs_floor`` flags the matrix; so does a second Gram matrix with an entry of G2 - I above ``orth_tol`` in modulus, which is
    what a first pass that lost its orthogonality to kappa^2 eps looks like.  A flagged matrix comes back unchanged."""
    a = np.array(a, dtype=np.complex128)
    q, k = a.copy(), a.shape[1]
    for second in (False, True):
        with np.errstate(all="ignore"):
            g = np.conj(q.T) @ q
            if second and not np.all(np.abs(g - np.eye(k)) <= orth_tol):
                return a, QR_RANK_DEFICIENT
            diag, low = np.real(np.diag(g)).copy(), np.zeros((k, k), dtype=np.complex128)
            for j in range(k):
                piv = g[j, j].real
                if not (piv > pivot_rel * diag[j]) or not (piv > abs_floor) or not np.isfinite(piv):
                    return a, QR_RANK_DEFICIENT
                low[j, j] = np.sqrt(piv)
                low[j + 1:, j] = g[j + 1:, j] / low[j, j]
                g[j + 1:, j + 1:] -= np.outer(low[j + 1:, j], np.conj(low[j + 1:, j]))
            x = np.zeros((k, k), dtype=np.complex128)          # L^-1 by forward substitution, a column at a time
            for c in range(k):
                x[c, c] = 1.0 / low[c, c]
                for i in range(c + 1, k):
                    x[i, c] = -(low[i, c:i] @ x[c:i, c]) / low[i, i]
            q = q @ np.conj(x.T)
    return q, 0


def extended_range_basis(a: np.ndarray) -> np.ndarray:
    """Orthonormal basis of the range of ``a`` by modified Gram-Schmidt, run twice, in x86 extended precision (np.clongdouble,
    eps 1.1e-19: the range is good to ~1e-19 kappa), rounded to complex128 at the end."""
    q = np.array(a, dtype=np.clongdouble)
    for _ in range(2):
        for j in range(q.shape[1]):
            for i in range(j):
                q[:, j] -= np.sum(np.conj(q[:, i]) * q[:, j]) * q[:, i]
            q[:, j] /= np.sqrt(np.sum(np.real(q[:, j]) ** 2 + np.imag(q[:, j]) ** 2))
    return q.astype(np.complex128)


def haar_isometry(m: int, n: int, rng) -> np.ndarray:
    """(m, n) with orthonormal columns, Haar: Q of a complex Gaussian with the phases of R's diagonal moved into Q."""
    q, r = np.linalg.qr(rng.standard_normal((m, n)) + 1j * rng.standard_normal((m, n)))
    ph = np.diag(r) / np.abs(np.diag(r))
    return q * ph


def kahan(d: int, k: int, theta: float, seed: int) -> np.ndarray:
    """A (d, k) Kahan matrix: R = diag(s^0 .. s^(k-1)) (I - c strict_upper_ones), c, s = cos, sin theta, times a Haar isometry
    from the left.  Its columns all have norm 1 to O(1), every Cholesky pivot ratio is benign, and its condition number grows
    like (1 + c)^k: the matrices on which a per-column pivot test sees nothing."""
    c, s = np.cos(theta), np.sin(theta)
    r = (s ** np.arange(k))[:, None] * (np.eye(k) - c * np.triu(np.ones((k, k)), 1))
    return np.ascontiguousarray(np.linalg.qr(_gauss(np.random.default_rng(seed), d, k))[0] @ r)


def with_spectrum(m: int, n: int, s, rng) -> tuple:
    """(a, U, V) with a = U diag(s) V^H, U (m, k) and V (n, k) Haar isometries, k = min(m, n) = len(s)."""
    s = np.asarray(s, dtype=float)
    u, v = haar_isometry(m, len(s), rng), haar_isometry(n, len(s), rng)
    return np.ascontiguousarray((u * s) @ np.conj(v.T)), u, v


def cond_equilibrated(a: np.ndarray) -> float:
    """2-norm condition number of ``a`` with its columns scaled to norm 1 (in extended precision before the SVD)."""
    al = np.array(a, dtype=np.clongdouble)
    al = al / np.sqrt(np.sum(np.real(al) ** 2 + np.imag(al) ** 2, axis=0))
    sv = np.linalg.svd(al.astype(np.complex128), compute_uv=False)
    return float(sv[0] / sv[-1]) if sv[-1] > 0 else float("inf")


def straddling_family():
    """(name, matrix) over a family that crosses the QR's status rule: Kahan matrices at theta = 0.50 .. 1.40 in three shapes
    (kappa_eq from 3e2 to beyond 1e17) and geometric spectra of condition 1e6 .. 1e12."""
    for d, k in ((64, 64), (64, 32), (256, 64)):
        for theta in np.arange(50, 141, 5) / 100.0:
            yield f"kahan {d}x{k} theta={theta:.2f}", kahan(d, k, theta, seed=7)
    for e in range(6, 13):
        yield f"geometric 100x16 kappa=1e{e}", with_spectrum(100, 16, np.geomspace(1.0, 10.0 ** -e, 16), np.random.default_rng(e))[0]


def _gauss(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def generate(kind: int, target: np.ndarray, k: int, *, om=None, idx=None, vh_mul=None) -> tuple:
    """(X, Y = U X) of one lane: ``om`` the draw (rand, eigen), ``idx`` the k column indices (alt), ``vh_mul`` the map
    M -> V(thetas)^H M (eigen).  Householder QR: the objective does not depend on the basis chosen for the range."""
    d = target.shape[0]
    if kind == SKETCH_ALT:
        x = np.zeros((d, k), dtype=np.complex128)
        x[np.asarray(idx), np.arange(k)] = 1
    elif kind == SKETCH_RAND:
        x = np.linalg.qr(om)[0]
    else:
        x = np.linalg.qr(vh_mul(om) - np.conj(target.T) @ om)[0]
    return x, target @ x


def adam_walk(fun_grad, x0, niter: int, lr: float, beta1=0.9, beta2=0.99, eps=1e-8, tol=1e-6):
    """optimizer._adam with the evaluations numbered: fun_grad(x, s) = (fobj, grad) under sketch number s (1-based).  Iteration t
    evaluates at x_{t-1} under sketch t; the final cost is taken at x_final under sketch nit + 1.  Returns (x, profile of the
    nit + 1 values, nit, the nit + 1 points evaluated)."""
    x, m, v = np.array(x0, dtype=float), np.zeros(len(x0)), np.zeros(len(x0))
    prof, pts, t = [], [], 0
    for t in range(1, niter + 1):
        f, g = fun_grad(x, t)
        prof.append(f)
        pts.append(x.copy())
        m = beta1 * m + (1 - beta1) * g
        v = beta2 * v + (1 - beta2) * g * g
        step = lr * np.sqrt(1 - beta2**t) / (1 - beta1**t) * m / (np.sqrt(v) + eps)
        x = x - step
        if np.linalg.norm(step) < tol:
            break
    prof.append(fun_grad(x, t + 1)[0])
    pts.append(x.copy())
    return x, np.array(prof), t, pts
