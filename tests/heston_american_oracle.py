"""NumPy oracle of the American option under Heston (include/olha.h), independent of the device code.  A helper, not a test module.

american_from_state is AmericanOption.price's loop (oracle/numpy_reference.py american_from_paths, exotic_options.py:259-306) with the
regression on all monomials of the date's state, solved by np.linalg.lstsq (an SVD) on the monomials of (S_t / K, v_t / theta): on
purpose another parametrisation and another solver than the device's normal equations in standardised regressors.  Both span the same
polynomial space, so in exact arithmetic they make the same exercise decisions; the smallest exercise margin the oracle reports says
how far a case is from a decision that rounding could flip.  Raw powers of (S_t, v_t) are NOT used: lstsq's default cut-off drops
directions of that badly scaled design matrix and changes decisions.

normal_equations_fit restates the device's solve (elimination in the natural order, the pin rule) for the CPU tests that measure how
far the two solvers' continuation values lie apart.
"""
import numpy as np

MODELS = {                         # kappa, theta, sigma_v, rho, v0: the five models of the prototype
    "usual": (2.0, 0.04, 0.3, -0.7, 0.04),
    "calm": (1.5, 0.09, 0.1, -0.5, 0.1),
    "high-vol-of-vol": (2.0, 0.04, 0.8, -0.7, 0.04),          # Feller's condition violated: many v = 0
    "extreme": (1.0, 0.04, 1.0, -0.9, 0.04),
    "fast-reversion": (6.0, 0.02, 0.4, 0.3, 0.06),
}


def monomials(x, y, degree):
    """Columns x^a y^b, a + b <= degree, in graded order 1, x, y, x^2, xy, y^2, ...; y=None keeps the powers of x alone."""
    if y is None:
        return np.column_stack([x**a for a in range(degree + 1)])
    return np.column_stack([x**(s - b) * y**b for s in range(degree + 1) for b in range(s + 1)])


def lstsq_fit(A, cf):
    return np.linalg.lstsq(A, cf, rcond=None)[0]


def normal_equations_fit(A, cf, report=None):
    """A^T A beta = A^T cf by elimination in the natural order; a pivot not above 1e-11 of its own diagonal moment pins that unknown.
    `report` (a list) receives per pivot (its ratio to its diagonal moment, the smallest ratio among the pivots of this solve that were
    divided by before it, 1.0 when none): what a caller needs to say how far a pin decision was from depending on rounding."""
    n = A.shape[1]
    aug = np.column_stack([A.T @ A, A.T @ cf])
    diag = np.diag(aug).copy()
    floor = 1.0
    for k in range(n):
        pinned = not abs(aug[k, k]) > 1e-11 * abs(diag[k])
        if report is not None:
            ratio = abs(aug[k, k]) / abs(diag[k]) if diag[k] else 0.0
            report.append((ratio, floor))
            floor = floor if pinned else min(floor, ratio)
        if pinned:
            aug[k, :] = 0.0
            aug[:, k] = 0.0
            aug[k, k] = 1.0
        aug[k + 1:, k + 1:] -= np.outer(aug[k + 1:, k] / aug[k, k], aug[k, k + 1:])
    beta = np.zeros(n)
    for k in range(n - 1, -1, -1):
        beta[k] = (aug[k, n] - aug[k, k + 1:n] @ beta[k + 1:]) / aug[k, k]
    return beta


def american_from_state(spot, var, K, T, r, theta, option_type="put", poly_degree=2, *, regressors=None, fit=lstsq_fit, with_variance=True,
                        return_decisions=False):
    """(price, the per-path time-0 cash flows, the smallest |intrinsic - continuation| over all in-the-money paths and fitted dates) from
    the (n_paths, n_steps + 1) matrices.  regressors(t, S_t, v_t) -> (x, y) replaces (S_t / K, v_t / theta); with return_decisions also
    the boolean (n_paths, n_steps + 1) matrix of the exercise decisions."""
    n_steps = spot.shape[1] - 1
    discount = np.exp(-r * (T / n_steps))
    intrinsic = np.maximum(spot - K, 0) if option_type == "call" else np.maximum(K - spot, 0)
    cf = intrinsic[:, -1].copy()
    margin = np.inf
    decisions = np.zeros(spot.shape, dtype=bool)
    for t in range(n_steps - 1, 0, -1):
        cf = cf * discount
        itm = intrinsic[:, t] > 0
        x, y = regressors(t, spot[itm, t], var[itm, t]) if regressors else (spot[itm, t] / K, var[itm, t] / theta)
        A = monomials(x, y if with_variance else None, poly_degree)
        if np.sum(itm) > A.shape[1]:
            cont = A @ fit(A, cf[itm])
            margin = min(margin, float(np.min(np.abs(intrinsic[itm, t] - cont))))
            idx = np.where(itm)[0][intrinsic[itm, t] > cont]
            cf[idx] = intrinsic[idx, t]
            decisions[idx, t] = True
    cf = cf * discount
    out = (float(np.mean(cf)), cf, margin)
    return out + (decisions,) if return_decisions else out
