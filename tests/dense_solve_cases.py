"""ekf_dense64_solve / ekf_dense64_color as include/ekfslam.h defines them: op-by-op float64 numpy models of the backward
substitution and of the colouring product, and the derived componentwise bounds they are tested against.  The families, the
sizes and the bit comparison are dense_factor_cases's."""
import numpy as np

from dense_factor_cases import (BLOCK_SIDES, U, gamma, integer_factor, np_factor, np_whiten, same_bits, sizes,  # noqa: F401
                                slam_like, slam_like_input)


def np_back(L, Y):
    """X[r] = L^-T Y[r]: x_i = (y_i - sum_{k>i} L[k][i] x_k) / L[i][i], i descending, k descending"""
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    X = np.zeros_like(Y)
    Na = L.shape[0]
    for i in range(Na - 1, -1, -1):
        s = Y[:, i].copy()
        for k in range(Na - 1, i, -1):
            s = s - L[k, i] * X[:, k]
        X[:, i] = s / L[i, i]
    return X


def np_color(L, Z, state=None):
    """X[r][i] = sum_{k<=i} L[i][k] Z[r][k], k ascending from 0.0; the state is added last.  Reads L[i][k] with k <= i only."""
    Z = np.atleast_2d(np.asarray(Z, dtype=np.float64))
    X = np.zeros_like(Z)
    for i in range(L.shape[0]):
        s = np.zeros(Z.shape[0])
        for k in range(i + 1):
            s = s + L[i, k] * Z[:, k]
        X[:, i] = s if state is None else s + state[i]
    return X


def same_up_to_zero_sign(a, b):
    """bit for bit, but +0.0 and -0.0 are the same value"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return same_bits(a + 0.0, b + 0.0)


# ---- the derived bounds (Higham, Accuracy and Stability of Numerical Algorithms, Theorems 8.5, 3.1 / 3.5 and 10.4:
# componentwise, valid for any order of summation and with fused multiply-adds; every product below is formed in extended
# precision, whose own error is 2^-11 of the bound at most) -----------------------------------------------------------------

def _x(a):
    return np.asarray(a, dtype=np.longdouble)


def _lower(L):
    return np.tril(np.asarray(L, dtype=np.float64))


def back_residual_ratio(L, x, y):
    """max_i |L^T x - y|_i / (gamma_Na (|L^T| |x|)_i)"""
    Lx = _x(_lower(L))
    res = np.abs(Lx.T @ _x(x) - _x(y))
    bound = np.longdouble(gamma(L.shape[0])) * (np.abs(Lx).T @ np.abs(_x(x)))
    return float(np.max(res / bound))


def color_residual_ratio(L, x, z, state=None):
    """max_i |x - L z (- state)|_i / (gamma_n (|L| |z| (+ |state|))_i), n = Na, or Na + 1 with the state: the addition is one
    more rounded operation on the same sum"""
    Lx, Na = _x(_lower(L)), L.shape[0]
    exact, mag = Lx @ _x(z), np.abs(Lx) @ np.abs(_x(z))
    if state is not None:
        exact, mag = exact + _x(state), mag + np.abs(_x(state))
    bound = np.longdouble(gamma(Na + (state is not None))) * mag
    return float(np.max(np.abs(_x(x) - exact) / bound))


def solve_residual_ratio(A, L, x, b):
    """max_i |A x - b|_i / (gamma_{3 Na + 1} (|L| |L^T| |x|)_i), A the symmetric matrix that was factored"""
    Lx, Na = _x(_lower(L)), L.shape[0]
    res = np.abs(_x(A) @ _x(x) - _x(b))
    bound = np.longdouble(gamma(3 * Na + 1)) * (np.abs(Lx) @ (np.abs(Lx).T @ np.abs(_x(x))))
    return float(np.max(res / bound))
