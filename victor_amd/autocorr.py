"""Integrated autocorrelation times and effective sample sizes of the chains of ``sample_chains``: the ``autocorr=`` keyword
(``CCFFit``, ``Realisations``, ``JointFit``, ``JointRealisations`` and the ``evaluate=`` route).

With ``keep_chain=False`` a run keeps no history, ``rhat`` is None, and under the stretch move it is None by design: nothing says
how many independent samples stand behind a pooled mean, a histogram or an interval.  The series whose autocorrelation answers
that is the per-step mean over a problem's W chains (walkers) - what emcee recommends for an ensemble - and its lagged products
up to a fixed lag need no history: they are accumulated where the chains run, on the device by a small kernel behind the step
kernel of every kept step (``vk_chain_set_autocorr``, ``victor_amd/csrc/vk_autocorr.h``), on the definition route by
:class:`SeriesState` below.  Three implementations - the device, a g++ build of the header, NumPy - agree bit for bit, because
every rounding is fixed:

**The series value** of a kept step (a kept sweep, after its second half), per problem r and sampled parameter j, is the SUM of
``x[rW + w, j]`` over the W chains in this shape: lane l of 64 starts from +0.0 and adds w = l, l + 64, ... in increasing w; six
halvings ``v[:h] + v[h:]`` of the 64 partials follow (the lanes' xor butterfly).  No division by W: the autocorrelation does not
depend on scale.  **The value**: at the first kept step (n = 0) the pivot is p = s and a_0 = 0; afterwards a_n = s - p.
**The state** per series: ``pivot``, ``total`` (sum of a_t), ``head[L]`` (a_0 .. a_{L-1}), ``ring[L]`` (slot u mod L holds a_u),
``acc[L]``.  **Kept step n**: ``acc[k] += a_n * a_{n-k}`` for 0 <= k <= min(n, L - 1), product and sum each rounded; ``total +=
a_n``; ``head[n] = a_n`` while n < L; ``ring[n mod L] = a_n``.

**The read-out** (:class:`Autocorr`) is formed in extended precision: mu = total / n, H_k the sum of the first k head values,
Z_k the sum of the last k ring values, ``n c_k = acc[k] - mu (2 total - H_k - Z_k) + (n - k) mu^2``, rho_k = c_k / c_0 - in exact
arithmetic the estimator of :func:`sokal_tau` on the history.  Sokal's window: tau(M) = 2 sum_{k <= M} rho_k - 1 at the smallest
M >= c tau(M); when no M <= L - 1 qualifies tau is NaN and ``reached`` False (raise ``max_lag`` or ``thin``).  ``ess = W n / tau``;
tau counts kept steps (kept sweeps).  The state costs (3 L + 2) R d doubles: about 63 MB at R = 1024, d = 10, L = 256.
"""

import numpy as np

from .utils import InputError

LANES = 64
MAX_LAG = 1024
DEFAULT_MAX_LAG, DEFAULT_C = 128, 5.0


def series_sum(x, R, W):
    """The series value (R, d) of the positions ``x`` (R W, d), chain c = r W + w: the lane sums and the halvings of the module
    docstring."""
    x = np.asarray(x, dtype=np.float64)
    d = x.shape[-1]
    rows = -(-W // LANES)
    padded = np.zeros((R, rows * LANES, d))
    padded[:, :W] = x.reshape(R, W, d)
    v = np.zeros((R, LANES, d))
    for i in range(rows):
        v = v + padded[:, i * LANES:(i + 1) * LANES]
    h = LANES // 2
    while h:
        v = v[:, :h] + v[:, h:]
        h //= 2
    return v[:, 0]


class SeriesState:
    """The running state of R d series of W chains each with L lags - the NumPy definition of what ``vk_chain_series_kernel``
    keeps: ``pivot``, ``total`` (R, d), ``head``, ``ring``, ``acc`` (R, d, L) and the count ``n`` of kept steps added."""

    FIELDS = ("pivot", "total", "head", "ring", "acc")

    def __init__(self, R, d, W, L):
        self.R, self.d, self.W, self.L = int(R), int(d), int(W), int(L)
        self.n = 0
        self.pivot, self.total = np.zeros((R, d)), np.zeros((R, d))
        self.head, self.ring, self.acc = np.zeros((R, d, L)), np.zeros((R, d, L)), np.zeros((R, d, L))

    def add(self, x):
        """One kept step: the positions ``x`` (R W, d) of all chains."""
        n, L = self.n, self.L
        s = series_sum(x, self.R, self.W)
        if n == 0:
            self.pivot[...] = s
            a = np.zeros_like(s)
        else:
            a = s - self.pivot
        top = min(n, L - 1)
        self.acc[:, :, 0] = self.acc[:, :, 0] + a * a
        if top >= 1:
            k = np.arange(1, top + 1)
            prod = a[:, :, None] * self.ring[:, :, (n - k) % L]
            self.acc[:, :, 1:top + 1] = self.acc[:, :, 1:top + 1] + prod
        self.total = self.total + a
        if n < L:
            self.head[:, :, n] = a
        self.ring[:, :, n % L] = a
        self.n = n + 1
        return self

    def arrays(self):
        return {k: getattr(self, k).copy() for k in self.FIELDS}


def sokal_tau(series, c=5.0):
    """(tau, M) of a kept history: the integrated autocorrelation time of the 1-D ``series``, tau(M) = 2 sum_{t <= M} rho_t - 1
    at the smallest M >= c tau(M) (the last lag when none qualifies), with the autocorrelation from an FFT."""
    x = np.asarray(series, dtype=float) - np.mean(series)
    n = len(x)
    f = np.fft.rfft(x, 2 * n)
    acf = np.fft.irfft(f * np.conj(f))[:n]
    acf = acf / acf[0]
    taus = 2.0 * np.cumsum(acf) - 1.0
    ok = np.arange(n) >= c * taus
    m = int(np.argmax(ok)) if ok.any() else n - 1
    return float(taus[m]), m


def acf_from_state(n, total, head, ring, acc):
    """rho_k (..., L) in ``np.longdouble`` from the state of series that hold ``n`` values (module docstring); NaN at the lags
    k >= n, which no step has reached, and everywhere for n == 0."""
    ld = np.longdouble
    total, head, ring, acc = (np.asarray(a, dtype=ld) for a in (total, head, ring, acc))
    L = acc.shape[-1]
    rho = np.full(acc.shape, np.nan, dtype=ld)
    m = min(int(n), L)                                    # the lags 0 .. m - 1 have been reached
    if m < 1:
        return rho
    mu = (total / ld(n))[..., None]
    zero = np.zeros(acc.shape[:-1] + (1,), dtype=ld)
    recent = ring[..., (n - 1 - np.arange(m)) % L]        # a_{n-1}, a_{n-2}, ...
    H = np.concatenate([zero, np.cumsum(head[..., :m - 1], axis=-1)], axis=-1)
    Z = np.concatenate([zero, np.cumsum(recent[..., :m - 1], axis=-1)], axis=-1)
    k = np.arange(m).astype(ld)
    nc = acc[..., :m] - mu * (2 * total[..., None] - H - Z) + (ld(n) - k) * mu * mu
    with np.errstate(invalid="ignore", divide="ignore"):
        rho[..., :m] = nc / nc[..., :1]
    return rho


def sokal_window(rho, c):
    """(tau, window, reached) of autocorrelations ``rho`` (..., L): Sokal's window over the lags given; without a lag M >=
    c tau(M) tau is NaN, the window -1 and ``reached`` False."""
    rho = np.asarray(rho, dtype=np.longdouble)
    taus = 2 * np.cumsum(rho, axis=-1) - 1
    with np.errstate(invalid="ignore"):
        ok = np.arange(rho.shape[-1]) >= np.longdouble(c) * taus        # NaN: False
    reached = ok.any(axis=-1)
    window = np.where(reached, np.argmax(ok, axis=-1), -1)
    tau = np.take_along_axis(taus, np.maximum(window, 0)[..., None], axis=-1)[..., 0].astype(float)
    return np.where(reached, tau, np.nan), window, reached


class Autocorr:
    """What ``Chains.autocorr`` holds: ``tau`` (R, d) in kept steps (kept sweeps), ``window`` (R, d) (the lag M of Sokal's window;
    -1 where it was not reached), ``ess`` (R, d) = W n / tau, ``reached`` (R, d), ``acf`` (R, d, L) (NaN at lags no step has
    reached), ``names``, ``n`` (kept steps), ``max_lag``, ``c`` and ``state``: the raw arrays ``pivot``, ``total`` (R, d),
    ``head``, ``ring``, ``acc`` (R, d, L) as the route that ran the chains returns them."""

    def __init__(self, names, W, n, c, state):
        self.names, self.n, self.c = list(names), int(n), float(c)
        self.state = {k: np.array(state[k], dtype=np.float64) for k in SeriesState.FIELDS}
        self.max_lag = self.state["acc"].shape[-1]
        rho = acf_from_state(self.n, *(self.state[k] for k in ("total", "head", "ring", "acc")))
        self.tau, self.window, self.reached = sokal_window(rho, self.c)
        self.acf = rho.astype(float)
        with np.errstate(invalid="ignore", divide="ignore"):
            self.ess = W * self.n / self.tau


def resolve_autocorr(autocorr, who):
    """(max_lag, c) of an ``autocorr=`` argument, None for None or False; every refusal is an :class:`InputError`, raised before
    any evaluation."""
    if autocorr is None or autocorr is False:
        return None
    if autocorr is True:
        autocorr = {}
    if not isinstance(autocorr, dict):
        raise InputError(f"{who}: autocorr must be None, True or a dict with the keys max_lag, c")
    opt = dict(autocorr)
    L, c = opt.pop("max_lag", DEFAULT_MAX_LAG), opt.pop("c", DEFAULT_C)
    if opt:
        raise InputError(f"{who}: autocorr has unknown keys {sorted(opt)} (max_lag, c)")
    if isinstance(L, bool) or not isinstance(L, (int, np.integer)) or not 1 <= L <= MAX_LAG:
        raise InputError(f"{who}: autocorr max_lag must be an integer in 1..{MAX_LAG}, not {L!r}")
    if isinstance(c, bool) or not isinstance(c, (int, float, np.integer, np.floating)) or not (c > 0 and np.isfinite(c)):
        raise InputError(f"{who}: autocorr c must be a finite number > 0, not {c!r}")
    return int(L), float(c)
