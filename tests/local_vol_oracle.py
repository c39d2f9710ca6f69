"""NumPy restatement of the local-volatility recursion of include/olmc_local_vol.h, given its normals (not a test module).

    x_0 = 0;  sigma_t = vol(x_t, t dt);  x_{t+1} = x_t + (r - q - sigma_t^2 / 2) dt + sigma_t sqrt(dt) z_t;  S_t = S exp(x_t)

`vol` is the header's bilinear lookup on a uniform table A[n_t][n_x], held flat beyond every edge; the nodes are rounded to fp32 as the
library rounds them when it uploads the table, the arithmetic is fp64.  Checked against closed forms by tests/test_local_vol_cpu.py.
"""
import numpy as np


class Table:
    """vol[n_t][n_x] over x in [x_lo, x_hi] (columns) and tau in [0, t_hi] (rows); a 1-D vol is one row without a time axis."""

    def __init__(self, vol, x_lo, x_hi, t_hi=1.0):
        vol = np.asarray(vol, dtype=np.float64)
        self.vol = vol[None, :] if vol.ndim == 1 else vol
        self.x_lo, self.x_hi, self.t_hi = float(x_lo), float(x_hi), float(t_hi)

    @property
    def args(self):
        """The (vol, x_lo, x_hi, t_hi) tuple optionslab_amd._hip's local-volatility calls take."""
        return self.vol, self.x_lo, self.x_hi, self.t_hi

    def lookup(self, x, tau):
        """sigma at (x, tau): x an array, tau a scalar (the time weights are the same for every path)."""
        a = self.vol.astype(np.float32).astype(np.float64)
        n_t, n_x = a.shape
        u = np.clip((np.asarray(x, dtype=np.float64) - self.x_lo) * (n_x - 1) / (self.x_hi - self.x_lo), 0.0, n_x - 1)
        j = np.minimum(np.floor(u).astype(np.int64), n_x - 2)
        w = u - j
        if n_t == 1:
            return a[0, j] + w * (a[0, j + 1] - a[0, j])
        v = min(max(tau * (n_t - 1) / self.t_hi, 0.0), n_t - 1.0)
        i = min(int(np.floor(v)), n_t - 2)
        w_tau = v - i
        a0 = a[i, j] + w * (a[i, j + 1] - a[i, j])
        a1 = a[i + 1, j] + w * (a[i + 1, j + 1] - a[i + 1, j])
        return a0 + w_tau * (a1 - a0)


def smile_table(n_t, n_x, x_lo, x_hi, t_hi):
    """The tests' smile: a skew and a term structure, 0.22 - 0.25 x + 0.4 x^2 + 0.05 tau / t_hi on the uniform grid."""
    x = np.linspace(x_lo, x_hi, n_x)[None, :]
    tau = (np.arange(n_t)[:, None] / max(n_t - 1, 1))
    return Table(0.22 - 0.25 * x + 0.4 * x * x + 0.05 * tau, x_lo, x_hi, t_hi)


def log_paths(z, table, T, r, q):
    """x[m, n + 1] from the normals z[m, n]."""
    z = np.asarray(z, dtype=np.float64)
    m, n = z.shape
    dt = T / n
    x = np.zeros((m, n + 1))
    for t in range(n):
        sigma = table.lookup(x[:, t], t * dt)
        x[:, t + 1] = x[:, t] + (r - q - 0.5 * sigma * sigma) * dt + sigma * np.sqrt(dt) * z[:, t]
    return x


def paths(z, table, S, T, r, q):
    """The spot matrix S exp(x), column 0 = S itself."""
    spot = S * np.exp(log_paths(z, table, T, r, q))
    spot[:, 0] = S
    return spot


def gbm_normals(spot, T, r, sigma, q):
    """The normals of a GBM path matrix spot[m, n + 1] of volatility sigma: its recursion solved for z, step by step."""
    n = spot.shape[1] - 1
    dt = T / n
    return (np.diff(np.log(spot), axis=1) - (r - q - 0.5 * sigma * sigma) * dt) / (sigma * np.sqrt(dt))


def payoff(spot, code, is_call, K, barrier=0.0):
    """The payoff of every row of a spot matrix for the codes of ollv_price: 0-3 barriers (up-out, up-in, down-out, down-in), 4 / 5
    floating / fixed lookback, 6 / 7 arithmetic / geometric Asian (mean over dates 1 .. n), 8 European.  Extrema run over dates 0 .. n."""
    sign = 1.0 if is_call else -1.0
    s_n, mx, mn = spot[:, -1], spot.max(axis=1), spot.min(axis=1)
    vanilla = np.maximum(sign * (s_n - K), 0.0)
    if code <= 3:
        crossed = mx >= barrier if code <= 1 else mn <= barrier
        return np.where(crossed if code in (1, 3) else ~crossed, vanilla, 0.0)
    if code == 4:
        return s_n - mn if is_call else mx - s_n
    if code == 5:
        return np.maximum(mx - K, 0.0) if is_call else np.maximum(K - mn, 0.0)
    if code == 6:
        return np.maximum(sign * (spot[:, 1:].mean(axis=1) - K), 0.0)
    if code == 7:
        return np.maximum(sign * (np.exp(np.log(spot[:, 1:]).mean(axis=1)) - K), 0.0)
    return vanilla
