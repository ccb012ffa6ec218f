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
