"""The NumPy statement of measuring an MPS (csrc/aqc_mps_sample_rule.h): what aqc_research_amd/mps_sampling.py and
csrc/aqc_mps_sample.hip are tested against.  Written with plain matrix products on mps_obs_ref.site_tensors / right_environments and
NumPy's own Philox, vectorised over the shots only; tests/test_mps_sample_ref.py holds it to the dense vector.

For shot s of lane l, with v = [1] and q = 0 .. n - 1:
    w_c = v T_q[c];  m_c = Re w_c R_{q+1} w_c^H;  u = uniform(seed, l, s, q);  bit = 0 if u (m_0 + m_1) < m_0 else 1;  v = w_bit
without rescaling; after the last site v is psi(b).  The margin of a shot is min over q of |u (m_0 + m_1) - m_0| / (m_0 + m_1): how far
the shot stays from every threshold, i.e. how large a relative error of the weights could change one of its bits."""
import numpy as np

from tests import mps_obs_ref

SAMPLE_STREAM = 16   # AQC_SAMPLE_STREAM of include/aqc_hip.h


def uniforms(seed: int, lane: int, shots, n: int) -> np.ndarray:
    """(len(shots), n): row k holds the n uniforms of shot number shots[k]."""
    out = np.empty((len(shots), n))
    key = np.array([seed, SAMPLE_STREAM], dtype=np.uint64)   # (arrays: a list with a word beyond 2^63 would pass through float64)
    for k, s in enumerate(shots):
        out[k] = np.random.Generator(np.random.Philox(key=key, counter=np.array([0, int(s), lane, 0], dtype=np.uint64))).random(n)
    return out


def walk(qiskit_mps, u: np.ndarray):
    """(bits uint8 (S, n), amplitudes complex (S,), margins (S,)) of the shots whose uniforms are the rows of ``u``."""
    ts = mps_obs_ref.site_tensors(qiskit_mps)
    right = mps_obs_ref.right_environments(ts)
    shots, n = u.shape
    v = np.ones((shots, 1), dtype=np.complex128)
    bits = np.empty((shots, n), dtype=np.uint8)
    margin = np.full(shots, np.inf)
    for q in range(n):
        w = [v @ ts[q][c] for c in (0, 1)]
        m = [np.einsum("su,uv,sv->s", wc, right[q + 1], wc.conj()).real for wc in w]
        tot = m[0] + m[1]
        if not (np.all(np.isfinite(tot)) and np.all(tot > 0.0)):
            raise ValueError(f"site {q}: the weights of the two branches do not add up to a finite positive number")
        bits[:, q] = np.where(u[:, q] * tot < m[0], 0, 1)
        margin = np.minimum(margin, np.abs(u[:, q] * tot - m[0]) / tot)
        v = np.where(bits[:, q, None] == 0, w[0], w[1])
    return bits, v[:, 0], margin


def sample(qiskit_mps, shots, *, seed: int, lane: int = 0):
    """``shots``: a count (shots 0 .. shots - 1) or the shot numbers themselves."""
    numbers = range(shots) if isinstance(shots, (int, np.integer)) else shots
    n = len(qiskit_mps[0])
    return walk(qiskit_mps, uniforms(seed, lane, numbers, n))


def amplitudes(qiskit_mps, bits) -> np.ndarray:
    ts = mps_obs_ref.site_tensors(qiskit_mps)
    bits = np.asarray(bits)
    v = np.ones((bits.shape[0], 1), dtype=np.complex128)
    for q, t in enumerate(ts):
        v = np.where(bits[:, q, None] == 0, v @ t[0], v @ t[1])
    return v[:, 0]


def indices(bits) -> np.ndarray:
    """The dense-vector index of every row: bit q is qubit q."""
    bits = np.asarray(bits)
    return (bits.astype(np.int64) << np.arange(bits.shape[1], dtype=np.int64)[None, :]).sum(axis=1)


# the cases the GPU test samples (tests/test_hip_mps_sampling.py) and test_mps_sample_ref.py asserts the margin condition for
PHILOX_SEED = 2024
NORM = 1.7
PROFILE_40 = [1, 2, 4, 8] + [16] * 33 + [8, 4, 2, 1]
CASES = {   # name -> (bond dimensions, hand_made seed)
    "A": (mps_obs_ref.PROFILE_A, 11), "C": (mps_obs_ref.PROFILE_C, 12), "D": (mps_obs_ref.PROFILE_D, 13),
    "B13": (mps_obs_ref.profile_b(13), 14), "N40": (PROFILE_40, 15), "B2": (mps_obs_ref.profile_b(2), 16),
}
MARGIN = 1e-9


def case(name):
    dims, seed = CASES[name]
    return mps_obs_ref.hand_made(dims, seed, norm=NORM)
