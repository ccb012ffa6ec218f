"""NumPy statement of the batched block-Jacobi SVD (csrc/aqc_svd_batch.hip, csrc/aqc_svd_blocks.h): the columns of the work matrix in
blocks of 16, block pairs met in the order of the circle-method tournament (a bye when the block count is odd), and per pair the
Gram matrix of the panel, its diagonalisation by cyclic two-sided Jacobi and the resulting unitary applied to the panel's columns of W
and V, after one Newton-Schulz step J <- J + J (1 - J^H J) / 2 that takes the rounding of the rotations out of J.  The convergence test
is the one of the scalar routes, |g_pq|^2 <= tol^2 g_pp g_qq on the panel's fresh Gram matrix, with the same rule for numerically zero
columns.  There is no closing step of scalar sweeps: test_svd_block_host.py says why none is needed."""
import numpy as np

BLOCK, MAX_SWEEPS, INNER_SWEEPS = 16, 60, 2          # kSvdbBlock, kSvdbMaxSweeps, kSvdbInnerSweeps
TOL, NEGLIGIBLE2 = 1e-15, 1e-30                        # jacobi_svd's tol; kNegligible2 of csrc/aqc_mps_dev.h
CONVERGED, SWEEP_LIMIT, NON_FINITE = 0, 1, 2           # status values of aqc_svd_batch


def blocks(cols: int) -> int:
    return 0 if cols < 1 else (cols + BLOCK - 1) // BLOCK


def block_width(b: int, cols: int) -> int:
    return min(BLOCK, cols - b * BLOCK) if 0 <= b < blocks(cols) else 0


def schedule(nb: int) -> list:
    """rounds of (x, y) block pairs, y = -1: a bye (svdb_rounds, svdb_slots, svdb_pair)."""
    n2 = nb + (nb & 1)
    ring = n2 - 1
    out = []
    for r in range(max(ring, 1 if nb > 0 else 0)):
        pairs = []
        for slot in range(max(n2 // 2, 1)):
            a, b = (r % ring, ring) if slot == 0 else ((r + slot) % ring, (r + ring - slot) % ring)
            a, b = min(a, b), max(a, b)
            pairs.append((a, b if b < nb else -1))
        out.append(pairs)
    return out


def _rotations(a, b, g, negligible):
    """(rotate?, c, se) of the 2x2 Hermitian [[a, g], [conj(g), b]] -- vectorised over pairs."""
    g2 = g.real**2 + g.imag**2
    rot = (g2 > TOL * TOL * a * b) & (g2 != 0.0) & (np.minimum(a, b) > negligible)
    with np.errstate(all="ignore"):
        d = b - a
        h = np.sqrt(d * d + 4.0 * g2)
        u2 = 2.0 / (np.abs(d) + h)
        c = 1.0 / np.sqrt(1.0 + g2 * u2 * u2)
        f = np.where(d >= 0.0, c * u2, -c * u2)
    return rot, np.where(rot, c, 1.0), np.where(rot, f * np.conj(g), 0.0)


def _inner_pairs(n: int, r: int):
    ring = n - 1
    p = [r % ring] + [(r + s) % ring for s in range(1, n // 2)]
    q = [ring] + [(r + ring - s) % ring for s in range(1, n // 2)]
    p, q = np.minimum(p, q), np.maximum(p, q)
    return np.asarray(p), np.asarray(q)


def diagonalise(g: np.ndarray, valid: np.ndarray, negligible: float, newton_schulz: bool = True) -> tuple:
    """Cyclic two-sided Jacobi on the Hermitian 32 x 32 ``g`` (entries of columns that do not exist are zero and never rotate):
    (J, rotated) with J^H g J diagonal to the relative criterion, or after INNER_SWEEPS sweeps, J after one Newton-Schulz step."""
    n = g.shape[0]
    g, j = g.copy(), np.eye(n, dtype=np.complex128)
    any_rot = False
    for _ in range(INNER_SWEEPS):
        swept = False
        for r in range(n - 1):
            p, q = _inner_pairs(n, r)
            rot, c, se = _rotations(g[p, p].real, g[q, q].real, g[p, q], negligible)
            rot &= valid[p] & valid[q]
            if not rot.any():
                continue
            swept = True
            c, se = np.where(rot, c, 1.0), np.where(rot, se, 0.0)
            for mat in (g, j):                                   # columns: x' = c x - se y, y' = conj(se) x + c y
                x, y = mat[:, p].copy(), mat[:, q].copy()
                mat[:, p], mat[:, q] = c * x - se * y, np.conj(se) * x + c * y
            x, y = g[p, :].copy(), g[q, :].copy()                # rows: the conjugate
            g[p, :], g[q, :] = c[:, None] * x - np.conj(se)[:, None] * y, se[:, None] * x + c[:, None] * y
            g[p[rot], q[rot]] = 0.0
            g[q[rot], p[rot]] = 0.0
            g[p, p], g[q, q] = g[p, p].real, g[q, q].real
        any_rot |= swept
        if not swept:
            break
    if any_rot and newton_schulz:   # (False: only to show what the step is for, see __main__)
        j = j + 0.5 * (j @ (np.eye(n) - np.conj(j.T) @ j))
    return j, any_rot


def svd_block(a: np.ndarray, newton_schulz: bool = True) -> tuple:
    """(u, s, vh, sweeps, status) of one complex matrix by the block rule."""
    a = np.asarray(a, dtype=np.complex128)
    m, n = a.shape
    k = min(m, n)
    if not np.all(np.isfinite(a)):
        return np.zeros((m, k), complex), np.zeros(k), np.zeros((k, n), complex), 0, NON_FINITE
    mode = 1 if n > m else 0
    w = np.array(np.conj(a.T) if mode else a, dtype=np.complex128)
    rows, cols = w.shape
    v = np.eye(cols, dtype=np.complex128)
    negligible = NEGLIGIBLE2 * float(np.sum(w.real**2 + w.imag**2))
    nb = blocks(cols)
    sweeps, status = 0, SWEEP_LIMIT
    while sweeps < MAX_SWEEPS:
        sweeps += 1
        rotated = False
        for pairs in schedule(nb):
            for x, y in pairs:
                idx = np.r_[np.arange(x * BLOCK, x * BLOCK + block_width(x, cols)), np.arange(y * BLOCK, y * BLOCK + block_width(y, cols))]
                loc = np.r_[np.arange(block_width(x, cols)), BLOCK + np.arange(block_width(y, cols))]
                valid = np.zeros(2 * BLOCK, dtype=bool)
                valid[loc] = True
                g = np.zeros((2 * BLOCK, 2 * BLOCK), dtype=np.complex128)
                g[np.ix_(loc, loc)] = np.conj(w[:, idx].T) @ w[:, idx]
                g = np.triu(g, 1) + np.conj(np.triu(g, 1).T) + np.diag(np.diag(g).real)
                dg = np.diag(g).real
                off = np.abs(np.triu(g, 1)) ** 2
                need = (off > TOL * TOL * np.outer(dg, dg)) & (off != 0.0) & (np.minimum.outer(dg, dg) > negligible)
                if not need.any():
                    continue
                jm, did = diagonalise(g, valid, negligible, newton_schulz)
                if not did:
                    continue
                rotated = True
                jj = jm[np.ix_(loc, loc)]
                w[:, idx] = w[:, idx] @ jj
                v[:, idx] = v[:, idx] @ jj
        if not rotated:
            status = CONVERGED
            break
    sigma = np.sqrt(np.sum(w.real**2 + w.imag**2, axis=0))
    order = np.argsort(-sigma, kind="stable")
    sigma, w, v = sigma[order], w[:, order], v[:, order]
    with np.errstate(all="ignore"):
        wn = np.where(sigma > 0.0, w / sigma, 0.0)
    if mode == 0:
        return wn, sigma, np.conj(v.T), sweeps, status
    return v, sigma, np.conj(wn.T), sweeps, status


if __name__ == "__main__":
    # python -m tests.svd_block_ref [m n case ...]: what the Newton-Schulz step on J is for, at the kernel's largest shapes (16 .. 80 s per
    # matrix, which is why no test runs this): |V V^H - 1| / (8 k eps) and the sweeps, without and with the step
    import sys

    from tests.helpers import maxdiff
    from tests.test_hip_svd_spectra import EPS, _input

    m, n = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (256, 128)
    for case in sys.argv[3:] or ["clusters", "graded", "graded-negligible"]:
        a, s_true = _input(case, m, n)[:2]
        for step in (False, True):
            u, s, vh, sweeps, status = svd_block(a, newton_schulz=step)
            good = s > 1e-12 * s_true[0]
            bound = 8 * min(m, n) * EPS
            print(f"{m} x {n} {case}, Newton-Schulz {step}: sweeps {sweeps}, status {status}, |s - s_true| / bound {maxdiff(s, s_true) / (bound * s_true[0]):.3f}, "
                  f"|V V^H - 1| / bound {maxdiff(vh[good] @ np.conj(vh[good].T), np.eye(int(good.sum()))) / bound:.3f}", flush=True)
