"""The NumPy statement of exact XXZ evolution: what csrc/aqc_xxz_rule.h and csrc/aqc_xxz.hip are tested against.

    H = -1/4 sum_{i=0}^{n-2} (X_i X_{i+1} + Y_i Y_{i+1} + delta Z_i Z_{i+1}),  open chain, index bit q = qubit q
    (H psi)(s) = -(delta/4) (n - 1 - 2 popcount(a(s))) psi(s) - 1/2 sum_{i: bit i of a(s)} psi(s ^ (3 << i)),  a(s) = (s ^ (s >> 1)) & (2^(n-1) - 1)
    exp(-iHt) psi = sum_{k=0}^{K} c_k T_k(H/R) psi,  x = R t,  R = (n-1)(1/2 + |delta|/4),  c_0 = J_0(x),  c_k = 2 (-i)^k J_k(x)
    K = the smallest k >= ceil(|x|) + 20 with |J_k(|x|)| <= 1e-17

Bessel values come from scipy.special.jv here; the library computes its own (Miller's recurrence)."""
import numpy as np
from scipy.special import jv


def dense_hamiltonian(n: int, delta: float) -> np.ndarray:
    """H by Kronecker products, the way the reference builds it (trotter.py:183-230)."""
    paulis = (np.array([[0, 1], [1, 0]], dtype=np.complex128), np.array([[0, -1j], [1j, 0]], dtype=np.complex128),
              np.array([[1, 0], [0, -1]], dtype=np.complex128))

    def full(s, j):
        return np.kron(np.kron(np.eye(2**j), s), np.eye(2 ** (n - j - 1)))

    h = np.zeros((2**n, 2**n), dtype=np.complex128)
    for weight, s in zip((1.0, 1.0, delta), paulis):
        for i in range(n - 1):
            h += weight * (full(s, i) @ full(s, i + 1))
    return -0.25 * h


def radius(n: int, delta: float) -> float:
    return (n - 1) * (0.5 + 0.25 * abs(delta))


def anti_mask(n: int) -> np.ndarray:
    s = np.arange(2**n, dtype=np.int64)
    return (s ^ (s >> 1)) & (2 ** (n - 1) - 1)


def mul_vec(psi: np.ndarray, delta: float) -> np.ndarray:
    """The matrix-free action on the last axis of ``psi`` ((2^n,) or (lanes, 2^n))."""
    dim = psi.shape[-1]
    n = dim.bit_length() - 1
    s = np.arange(dim, dtype=np.int64)
    a = anti_mask(n)
    pop = np.zeros(dim, dtype=np.int64)
    hop = np.zeros(psi.shape, dtype=np.complex128)
    for i in range(n - 1):
        on = ((a >> i) & 1).astype(bool)
        pop += on
        hop[..., on] += psi[..., s[on] ^ (3 << i)]
    return -(delta / 4) * (n - 1 - 2 * pop) * psi - 0.5 * hop


def series_length(x: float) -> int:
    ax = abs(float(x))
    k = int(np.ceil(ax)) + 20
    while abs(jv(k, ax)) > 1e-17:
        k += 1
    return k


def coefficients(x: float) -> np.ndarray:
    k = np.arange(series_length(x) + 1)
    c = 2.0 * np.array([1, -1j, -1, 1j])[k % 4] * jv(k, float(x))   # (-i)^k, exactly
    c[0] = jv(0, float(x))
    return c


def evolve(psi: np.ndarray, delta: float, t: float) -> np.ndarray:
    """exp(-iHt) psi by the series, for one state."""
    n = psi.shape[-1].bit_length() - 1
    r = radius(n, delta)
    c = coefficients(r * t)
    prev, cur = psi.astype(np.complex128), mul_vec(psi, delta) / r
    out = c[0] * prev + c[1] * cur
    for k in range(2, c.size):
        prev, cur = cur, (2.0 / r) * mul_vec(cur, delta) - prev
        out += c[k] * cur
    return out


def mul_vec_slices(psi: np.ndarray, delta: float) -> np.ndarray:
    """The same action written with slices instead of gathers, for the larger sizes of the GPU tests: bond i swaps |01> and |10>
    of bits (i + 1, i).  tests/test_xxz_ref.py holds it to ``mul_vec``."""
    dim = psi.shape[-1]
    n = dim.bit_length() - 1
    a = anti_mask(n)
    pop = np.zeros(dim, dtype=np.int64)
    for i in range(n - 1):
        pop += (a >> i) & 1
    hop = np.zeros(psi.shape, dtype=np.complex128)
    for i in range(n - 1):
        shape = psi.shape[:-1] + (2 ** (n - i - 2), 2, 2, 2**i)
        src, dst = psi.reshape(shape), hop.reshape(shape)
        dst[..., 0, 1, :] += src[..., 1, 0, :]
        dst[..., 1, 0, :] += src[..., 0, 1, :]
    return -(delta / 4) * (n - 1 - 2 * pop) * psi - 0.5 * hop


def evolve_lanes(states: np.ndarray, delta: float, times) -> np.ndarray:
    """Lane l: exp(-i H times[l]) of states[l], or of the one state when ``states`` is 1-D.  One loop to the longest series, the
    coefficients zero beyond a lane's own K -- the order in which the device runs it."""
    times = np.asarray(times, dtype=np.float64)
    n = states.shape[-1].bit_length() - 1
    r = radius(n, delta)
    cs = [coefficients(r * t) for t in times]
    c = np.zeros((max(v.size for v in cs), times.size), dtype=np.complex128)
    for lane, v in enumerate(cs):
        c[: v.size, lane] = v
    prev = np.ascontiguousarray(np.broadcast_to(states, (times.size, states.shape[-1])), dtype=np.complex128)
    cur = mul_vec_slices(prev, delta) / r
    out = c[0][:, None] * prev + c[1][:, None] * cur
    for k in range(2, c.shape[0]):
        prev, cur = cur, (2.0 / r) * mul_vec_slices(cur, delta) - prev
        out += c[k][:, None] * cur
    return out


def neel_index(n: int) -> int:
    return sum(1 << q for q in range(0, n, 2))


def random_states(n: int, lanes: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((lanes, 2**n)) + 1j * rng.standard_normal((lanes, 2**n))
    return np.ascontiguousarray(v / np.linalg.norm(v, axis=1, keepdims=True))
