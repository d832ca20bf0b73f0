"""The table contract of ``include/victor_hip.h`` (``vk_tables`` / ``vk_eval_opts``) evaluated in extended precision.

This is the specification the theory kernels implement, read off the tables they are handed (``engine.build_tables``) and
evaluated in ``np.longdouble`` (80-bit on x86-64, eps 1.1e-19): the same discrete operation the generic kernel performs
(``vk_common.h: point_scalars``, ``vk_kernel_generic.h``) - clamping to each table's box, interval choice, the PCHIP-in-beta
coefficient forms (extrapolating with the end pieces), the isotropic sigma_v table and the anisotropic bicubic patches,
streaming / dispersion / kaiser / euclid_special, ``assume_isotropic``, ``from_data``, ``empirical_corr``, the projection with
``w_ell`` and the Simpson weights ``w_x`` as stored, NaN inputs poisoning the row - and the chi-square side
(``vk_kernel_like.h``): the data at beta from its PCHIP pieces, the precision blend of ``CCFFit._bracket``, the log-determinant
term from ``logdet`` / ``eig``, the four likelihood forms and the failure semantics.

Only the ``vk_pp`` tables are read (``xi``, ``vr``, ``vr_emp``, ``sv``, ``sv2d``); the ``uni_*`` refinements are re-expansions
of the same cubics and their rounding belongs in the fast kernels' bound (``tests/tolerances.py``).  Both sides - the kernels
in FP64 and this module in longdouble - then evaluate one function, so ``|gpu - xp|`` is the kernel's own error, which
``tolerances.assert_theory_xp`` holds to a bound derived from the errors its arithmetic is documented to have.

Besides every entry of the theory vector, :meth:`XP.theory` returns what that bound needs, per entry: the magnitude of what was
summed (sum of ``|w_l w_x * integrand|``, with 1 + xi read as 1 + |xi|) and first-order sensitivities computed here by
longdouble finite differences (see :class:`Theory`).
"""

import numpy as np

from victor_amd import _native as N
from victor_amd import engine as E

LD = np.longdouble
assert np.finfo(LD).eps <= 1e-18, "tests/xp_reference.py needs an extended-precision np.longdouble (80-bit x87 on x86-64)"
_DELTA = LD(2) ** -26          # finite-difference step (relative): truncation ~1.5e-8, longdouble rounding ~1e-19 / 1.5e-8


def _arr(ptr, n):
    """A double array of the ctypes struct, as longdouble (exact)."""
    if n == 0 or not ptr:
        return None
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(LD)


def bracket(grid, beta):
    """(lo, t) of CCFFit._bracket on a covariance grid (vk_kernel_like.h: cov_bracket): below / above the grid the first /
    last slice, a grid value its slice (t = 0), else slice lo blended with the LAST slice by t; NaN beta gives t = NaN."""
    b = LD(beta)
    if not np.isfinite(b):
        return 0, LD(np.nan)
    if b < grid[0]:
        return 0, LD(0)
    if b > grid[-1]:
        return len(grid) - 1, LD(0)
    if np.any(grid == b):
        return int(np.nonzero(grid == b)[0][0]), LD(0)
    lo = int(np.nonzero(grid < b)[0][-1])
    return lo, (b - grid[lo]) / (grid[-1] - grid[lo])


def _horner(c, x):
    """sum_p c[..., p] x^p along the last axis of ``c``."""
    acc = c[..., -1]
    for p in range(c.shape[-1] - 2, -1, -1):
        acc = acc * x + c[..., p]
    return acc


class PP:
    """A clamped piecewise-cubic table on ``knots`` with coefficients ``coef[..., n_int, 4]`` (longdouble)."""

    def __init__(self, knots, coef):
        self.knots = knots
        self.coef = coef
        self.n_int = len(knots) - 1
        self.lo, self.hi = knots[0], knots[-1]

    def interval(self, u):
        """Clamped abscissa and the largest i with knots[i] <= u (vk_common.h: pp_interval)."""
        uc = np.minimum(np.maximum(u, self.lo), self.hi)
        i = np.clip(np.searchsorted(self.knots, uc, side="right") - 1, 0, self.n_int - 1)
        return uc, i, uc - self.knots[i]

    def __call__(self, var, u, at=None):
        uc, i, dx = self.interval(u) if at is None else at
        c = self.coef[var][i]
        return ((c[..., 3] * dx + c[..., 2]) * dx + c[..., 1]) * dx + c[..., 0]


def model_flags(model):
    """vk_eval_opts of a merged model option dictionary (engine.Engine.make_opts)."""
    return dict(rsd=N.RSD[model["rsd_model"]], iso=bool(model["assume_isotropic"]),
                ap=not model["velocity_independent_of_AP"], kaiser_approx=bool(model.get("kaiser_approximation", False)),
                coord_shift=bool(model.get("kaiser_coord_shift", True)), niter=int(model.get("niter", 5)),
                from_data=bool(model.get("realspace_ccf_from_data", False)),
                empirical=bool(model.get("empirical_corr", False)))


class Theory:
    """Per point (rows of :meth:`XP.theory`), every array (n, N) in the layout of the theory vector.

    - ``t``: the theory vector;
    - ``mag``: sum_i |W_l[i]| (sum_k |w_k f_ik| + 1), f with 1 + xi read as 1 + |xi| (and 1 + M xi - J as 1 + |M xi| + |J|);
    - ``s_ir``: sum_i |W_l[i]| sum_k |df_ik / d eps| for r -> r (1 + eps), mu_r -> mu_r (1 + eps) (a relative error of 1/r);
    - ``s_u``: the same for the table abscissa u = r / c alone (1/c, the AP integral, the fast kernels' interval coordinate);
    - ``s_rp``: the same for an absolute error of r_par of eps (|s_par| + |x_k B|) (the coordinate's own roundings);
    - ``s_z``: sum_i |W_l[i]| sum_k |z| (|z| + |z_v|) |w_k f_ik|, z the Gaussian's argument, z_v = A V mu_r / sigma its velocity
      part: a relative error eps of 1/sigma, A V or the exponent moves the integrand by at most eps times this;
    - ``s_fp`` (dispersion, kaiser / euclid_special with the coordinate shift): sum_i |W_l[i]| sum_k |df_ik / d eps| for
      r_par -> r_par (1 + eps) after the last pass, times the gain sum_{k=0}^{niter} rho^k of the fixed-point iteration (rho
      its relative contraction at the fixed point; niter + 1 passes, the rounding of pass j reaches the result through the
      niter - j passes after it): the response to a relative rounding eps in every pass, finite for any rho.
    """

    def __init__(self, **kv):
        self.__dict__.update(kv)


class XP:
    """The tables of a fit (one engine key: matter model, Simpson rule) and the evaluation of the contract on them."""

    def __init__(self, fit, kw=None):
        model = fit._merged(kw or {})
        self.model = model
        self.fit = fit
        key = fit._engine_key(model)
        rule = fit._simpson_rule(model["simpson_even"])
        t, keep = E.build_tables(fit, fit, key, rule)
        self._keep = (t, keep)
        L = E.table_array_lengths(t)
        g = lambda name, ptr: _arr(ptr, L[name])          # noqa: E731
        self.n_s, self.n_mu, self.n_x, self.n_ell = t.n_s, t.n_mu, t.n_x, t.n_ell
        self.s, self.mu, self.x, self.w_x = g("s", t.s), g("mu", t.mu), g("x", t.x), g("w_x", t.w_x)
        self.w_ell = g("w_ell", t.w_ell).reshape(t.n_ell, t.n_mu)
        self.n_ell_r, self.n_beta_r = t.n_ell_r, t.n_beta_r
        self.beta_r = g("beta_r", t.beta_r)
        nb = t.n_beta_r
        xk = g("xi.knots", t.xi.knots)
        xc = g("xi.coef", t.xi.coef)
        self.xi_knots = xk
        self.xi_coef = xc.reshape(t.n_ell_r, t.xi.n_int, 4) if nb == 0 else xc.reshape(t.n_ell_r, nb - 1, t.xi.n_int, 4, 4)
        self.matter_model = t.matter_model
        self.vr_beta_dep = t.vr_beta_dep
        vk = g("vr.knots", t.vr.knots)
        vc = g("vr.coef", t.vr.coef)
        self.vr_knots = vk
        self.vr_coef = vc.reshape(2, nb - 1, t.vr.n_int, 4, 4) if t.vr_beta_dep else vc.reshape(5, t.vr.n_int, 4)
        emp = g("vr_emp", t.vr_emp)
        self.vr_emp = emp.reshape(3, nb - 1, t.vr.n_int, 4, 7) if emp is not None else None
        self.vt_amp = LD(t.vt_amp)
        sk = g("sv.knots", t.sv.knots)
        self.sv_n_mu = t.sv_n_mu
        if t.sv_n_mu == 0:
            self.sv = PP(sk, g("sv.coef", t.sv.coef).reshape(1, t.sv.n_int, 4))
        else:
            self.sv = PP(sk, None)
            self.sv_mu = g("sv_mu", t.sv_mu)
            self.sv2d = g("sv2d", t.sv2d).reshape(t.sv.n_int, t.sv_n_mu - 1, 4, 4)
        self.iaH = LD(t.iaH)
        self.template_sigma8 = LD(t.template_sigma8)
        # data side
        self.N = t.n_ell * t.n_s
        self.n_beta_d = t.n_beta_d
        self.beta_d = g("beta_d", t.beta_d)
        d = g("data", t.data)
        self.data = d if t.n_beta_d == 0 else d.reshape(t.n_beta_d - 1, self.N, 4)
        self.n_beta_c = t.n_beta_c
        self.beta_c = g("beta_c", t.beta_c)
        P = g("prec", t.prec)
        self.prec = P.reshape(max(t.n_beta_c, 1), self.N, self.N)
        self.logdet = g("logdet", t.logdet)
        e = g("eig", t.eig)
        self.eig = e.reshape(t.n_beta_c, self.N) if e is not None else None
        self.like = fit._merged_fit(kw or {})["likelihood"] if hasattr(fit, "_merged_fit") else {"form": "Gaussian"}
        self.flags = model_flags(model)

    # ----------------------------------------------------------------------------------------------- per-point tables
    @staticmethod
    def beta_piece(grid, beta):
        """PCHIP piece k (last i in [1, n-2] with beta >= grid[i], else 0) and beta - grid[k] (build_beta_tables)."""
        k = 0
        for i in range(1, len(grid) - 1):
            if beta >= grid[i]:
                k = i
        return k, beta - grid[k]

    def point_tables(self, beta):
        """(xi PP with coef [l][i][4], vr PP with coef [5][i][4]) at this point's beta."""
        if self.n_beta_r == 0:
            xi = PP(self.xi_knots, self.xi_coef)
        else:
            k, db = self.beta_piece(self.beta_r, LD(beta))
            xi = PP(self.xi_knots, _horner(self.xi_coef[:, k], db))
        if not self.vr_beta_dep:
            vr = PP(self.vr_knots, self.vr_coef)
        else:
            k, db = self.beta_piece(self.beta_r, LD(beta))
            v = [_horner(self.vr_coef[0, k], db), _horner(self.vr_coef[1, k], db)]
            if self.vr_emp is not None:
                v += [_horner(self.vr_emp[j, k], db) for j in range(3)]
            else:
                v += [np.full_like(v[0], np.nan)] * 3
            vr = PP(self.vr_knots, np.stack(v))
        return xi, vr

    # ----------------------------------------------------------------------------------------------- point scalars
    def scalars(self, row):
        """vk_common.h: point_scalars (and growth_amplitude) in longdouble; ``poison`` is NaN for a bad input."""
        f = self.flags
        row = row.astype(LD)
        fs8, sigv, aperp, apar, eps = row[N.P_FSIGMA8], row[N.P_SIGMAV], row[N.P_APERP], row[N.P_APAR], row[N.P_EPSILON]
        if f["ap"]:
            h = (LD(1) - LD(1e-10)) / 49
            m = LD(1e-10) + np.arange(50, dtype=LD) * h
            m[-1] = LD(1)
            v = apar * np.sqrt((LD(1) - m * m) * (eps * eps - 1) + 1)
            v[0] *= LD(0.5)
            v[-1] *= LD(0.5)
            c = v.sum() * h
        else:
            c = row[N.P_ASTAR]
        growth = fs8 / self.template_sigma8
        binv = LD(1)
        extra = LD(0)
        if self.matter_model == N.MATTER["linear_bias"]:
            bias = row[N.P_BIAS]
            if f["from_data"]:
                growth = row[N.P_BETA] * bias
            binv = 1 / bias
            extra += bias
        if self.matter_model == N.MATTER["velocity_template"]:
            growth = -3 * self.iaH * self.vt_amp * fs8
        av = LD(0)
        if f["empirical"] and self.matter_model != N.MATTER["velocity_template"]:
            av = row[N.P_AV] * binv
            extra += av
        gb = growth * binv
        iaH_true = self.iaH * apar
        s = dict(aperp=aperp, apar=apar, c=c, B=sigv * iaH_true, A=gb / (3 * iaH_true * sigv), G=gb / 3, gD=gb / c,
                 M=row[N.P_M], Q=row[N.P_Q], av=av, beta=row[N.P_BETA])
        with np.errstate(invalid="ignore"):
            poison = 0 * (gb + sigv + aperp + apar + eps + c + s["A"] + extra + (row[N.P_BETA] if self.n_beta_r else 0))
        s["poison"] = poison
        return s

    # ----------------------------------------------------------------------------------------------- table shapes
    def sv_shape(self, u, mu_r):
        if self.sv_n_mu == 0:
            return self.sv(0, u)
        uc, i, du = self.sv.interval(u)
        mk = self.sv_mu
        m = np.minimum(np.maximum(mu_r, mk[0]), mk[-1])
        j = np.clip(np.searchsorted(mk, m, side="right") - 1, 0, len(mk) - 2)
        dm = m - mk[j]
        c = self.sv2d[i, j]                                         # [..., p, q]: du^p dmu^q
        cp = _horner(c, dm[..., None])                              # [..., p]
        return _horner(cp, du)

    def xi_real(self, xi, S, u, mu_r, r_par, s_perp, nlr):
        if self.flags["from_data"]:
            rp = r_par / S["apar"]
            rt = s_perp / S["aperp"]
            u = np.sqrt(rp * rp + rt * rt)
            mu_r = rp / u
        at = xi.interval(u)
        x = xi(0, None, at)
        if nlr > 1:
            m2 = mu_r * mu_r
            x = x + xi(1, None, at) * (LD(1.5) * m2 - LD(0.5))
            if nlr > 2:
                x = x + xi(2, None, at) * ((35 * m2 - 30) * m2 + 3) / 8
        return x

    # ----------------------------------------------------------------------------------------------- integrand
    def _final(self, S, xi, vr, nlr, s_perp, r_par, X, WX, pert=None, eps=LD(0)):
        """Integrand f (times w_x) at the coordinate r_par, and its magnitude / z factors.  ``pert`` names a perturbation of
        size ``eps`` (see Theory)."""
        f = self.flags
        rsd = f["rsd"]
        if pert == "rp":
            r_par = r_par + eps
        elif pert == "rpar":
            r_par = r_par * (1 + eps)
        r2 = s_perp * s_perp + r_par * r_par
        r = np.sqrt(r2)
        inv_r = 1 / r
        if pert == "ir":
            inv_r = inv_r * (1 + eps)
            r = r2 * inv_r
        mu_r = r_par * inv_r
        u = r / S["c"]
        if pert == "u":
            u = u * (1 + eps)
        at = vr.interval(u)
        V = vr(0, None, at)
        if f["empirical"]:
            V = V + S["av"] * vr(2, None, at)
        xir = self.xi_real(xi, S, u, mu_r, r_par, s_perp, nlr)
        one = LD(1)
        if rsd == N.RSD["streaming"]:
            SV = self.sv_shape(u, mu_r)
            inv_sv = one / SV
            zv = S["A"] * V * mu_r * inv_sv
            z = zv + X * inv_sv
            e = np.exp(-z * z / 2)
            g = WX * inv_sv * e
            return g * (1 + xir), g * (1 + np.abs(xir)), np.abs(z) * (np.abs(z) + np.abs(zv)) * np.abs(g * (1 + xir))
        q = -S["G"] * V * inv_r
        Dq = (vr(3, None, at) + S["av"] * vr(4, None, at)) if f["empirical"] else vr(1, None, at)
        dq = -S["gD"] * Dq
        m2 = mu_r * mu_r
        if rsd == N.RSD["dispersion"]:
            SV = self.sv_shape(u, mu_r)
            inv_sv = one / SV
            z = X * inv_sv
            jac = one / (1 + q + m2 * (dq - q))
            g = WX * jac * np.exp(-z * z / 2) * inv_sv
            return g * (1 + xir), np.abs(g) * (1 + np.abs(xir)), z * z * np.abs(g * (1 + xir))
        M, Q = S["M"], S["Q"]
        if rsd == N.RSD["kaiser"]:
            J = M * q + M * Q * m2 * (dq - q)
            if f["kaiser_approx"]:
                val = 1 + (M * xir - J)
                return val, 1 + np.abs(M * xir) + np.abs(J), np.zeros_like(val)
            val = (1 + M * xir) / (1 + J)
            return val, (1 + np.abs(M * xir)) / np.abs(1 + J), np.zeros_like(val)
        J = 3 * M * q + 2 * M * Q * m2 * (dq - q)
        val = 1 + (M * xir - J)
        return val, 1 + np.abs(M * xir) + np.abs(J), np.zeros_like(val)

    def _coordinate(self, S, vr, s_perp, s_par, X):
        """r_par of the integrand: s_par - x B (streaming), the fixed-point iteration (dispersion, kaiser / euclid_special
        with the coordinate shift), or s_par; and the relative contraction of the last pass (None without iteration)."""
        f = self.flags
        rsd = f["rsd"]
        if rsd == N.RSD["streaming"]:
            return s_par - X * S["B"], None
        disp = rsd == N.RSD["dispersion"]
        if not (disp or f["coord_shift"]):
            return s_par + 0 * X, None
        mfac = LD(1) if disp else S["M"]
        num = (s_par - X * S["B"]) if disp else s_par + 0 * X
        sp2 = s_perp * s_perp

        def q_of(r2):
            r = np.sqrt(r2)
            at = vr.interval(r / S["c"])
            V = vr(0, None, at)
            if f["empirical"]:
                V = V + S["av"] * vr(2, None, at)
            return -S["G"] * V / r

        def step(rp):
            return num / (1 + mfac * q_of(rp * rp + sp2))

        rp = num / (1 + mfac * q_of(s_par * s_par + sp2))
        for _ in range(f["niter"]):
            rp = step(rp)
        with np.errstate(invalid="ignore", divide="ignore"):
            hi, lo = step(rp * (1 + _DELTA)), step(rp * (1 - _DELTA))
            base = step(rp)
            rho = np.abs(hi - lo) / (2 * _DELTA * np.abs(base))
        rho = np.where(np.isfinite(rho), rho, 0)
        return rp, rho

    # ----------------------------------------------------------------------------------------------- public
    def _grid(self, s, mu, kais):
        s = np.asarray(s, dtype=np.float64).astype(LD)
        mu = np.asarray(mu, dtype=np.float64).astype(LD)
        smu = np.sqrt(1 - mu * mu)
        X = (np.zeros(1, LD) if kais else self.x)[None, None, :]
        WX = (np.ones(1, LD) if kais else self.w_x)[None, None, :]
        return s, mu, smu, X, WX

    def _cells(self, row, s, mu, sens):
        """Sums over the velocity nodes per (s, mu) cell: f, magnitude and sensitivities, each (n_s, n_mu)."""
        f = self.flags
        kais = f["rsd"] in (N.RSD["kaiser"], N.RSD["euclid_special"])
        s, mu, smu, X, WX = self._grid(s, mu, kais)
        S = self.scalars(np.asarray(row, dtype=np.float64))
        nlr = 1 if f["iso"] else self.n_ell_r
        shape = (len(s), len(mu))
        if not np.isfinite(S["poison"]):
            nan = np.full(shape, np.nan, dtype=LD)
            return dict(f=nan, mag=nan, s_ir=nan, s_u=nan, s_rp=nan, s_z=nan, s_fp=nan)
        xi, vr = self.point_tables(S["beta"])
        s_perp = (s[:, None, None] * S["aperp"]) * smu[None, :, None]
        s_par = (s[:, None, None] * S["apar"]) * mu[None, :, None]
        r_par, rho = self._coordinate(S, vr, s_perp, s_par, X)
        val, mag, z = self._final(S, xi, vr, nlr, s_perp, r_par, X, WX)
        out = dict(f=val.sum(-1), mag=mag.sum(-1) + 1)
        if sens:
            def d(pert, eps):
                with np.errstate(invalid="ignore", divide="ignore"):
                    v = self._final(S, xi, vr, nlr, s_perp, r_par, X, WX, pert, eps)[0]
                return np.abs(v - val)
            out["s_ir"] = (d("ir", _DELTA) / _DELTA).sum(-1)
            out["s_u"] = (d("u", _DELTA) / _DELTA).sum(-1)
            scale = np.abs(s_par) + np.abs(X * S["B"])
            out["s_rp"] = (d("rp", _DELTA * scale) / _DELTA).sum(-1)
            out["s_z"] = z.sum(-1)
            if rho is None:
                out["s_fp"] = np.zeros(shape, LD)
            else:
                gain = sum(rho ** k for k in range(self.flags["niter"] + 1))
                out["s_fp"] = (d("rpar", _DELTA) / _DELTA * gain).sum(-1)
        return out

    def theory(self, rows, sens=True):
        """Theory vectors of ``rows`` (n, VK_NPAR) on the fit's s grid and multipoles, as a :class:`Theory` of (n, N)
        longdouble arrays."""
        rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
        keys = ("t", "mag", "s_ir", "s_u", "s_rp", "s_z", "s_fp") if sens else ("t", "mag")
        res = {k: np.empty((len(rows), self.N), LD) for k in keys}
        W = self.w_ell
        aW = np.abs(W)
        wsum = W.sum(axis=1)
        for n, row in enumerate(rows):
            c = self._cells(row, self.s, self.mu, sens)
            res["t"][n] = (np.einsum("li,ji->lj", W, c["f"]) - wsum[:, None]).reshape(-1)
            for k in keys[1:]:
                res[k][n] = np.einsum("li,ji->lj", aW, c[k]).reshape(-1)
        return Theory(**res)

    def xi_smu(self, rows, s, mu, sens=True):
        """CCFModel.theory_xi on the (s, mu) grid (K1x): a :class:`Theory` of (n, n_mu, n_s) arrays (the sums run over the
        velocity nodes only)."""
        rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
        keys = ("t", "mag", "s_ir", "s_u", "s_rp", "s_z", "s_fp") if sens else ("t", "mag")
        res = {k: np.empty((len(rows), len(mu), len(s)), LD) for k in keys}
        for n, row in enumerate(rows):
            c = self._cells(row, s, mu, sens)
            res["t"][n] = (c["f"] - 1).T
            for k in keys[1:]:
                res[k][n] = c[k].T
        return Theory(**res)

    # ----------------------------------------------------------------------------------------------- chi-square
    def data_at(self, beta):
        if self.n_beta_d == 0:
            return self.data
        k, db = self.beta_piece(self.beta_d, LD(beta))
        return _horner(self.data[k], db)

    def bracket(self, beta):
        """(lo, t) of CCFFit._bracket on the covariance grid (NaN beta: t = NaN)."""
        return bracket(self.beta_c, beta)

    def precision(self, beta):
        """(P, lo, t) at beta."""
        if self.n_beta_c == 0:
            return self.prec[0], 0, LD(0)
        lo, t = self.bracket(beta)
        if t == 0:
            return self.prec[lo], lo, t
        return (1 - t) * self.prec[lo] + t * self.prec[-1], lo, t

    def log_det_factor(self, lo, t):
        """(-1/2 log det of the blended covariance, singular?) (vk_kernel_like.h: logdet_term)."""
        if self.n_beta_c == 0:
            return LD(0), False
        ld = self.logdet[lo]
        if t != 0:
            fct = (1 - t) + t * self.eig[lo]
            with np.errstate(divide="ignore", invalid="ignore"):
                ls = np.log(np.abs(fct)).sum()
            bad = bool(np.any((fct == 0) | ~np.isfinite(fct)))
            neg = int(np.sum(fct < 0))
        else:
            ls, bad, neg = LD(0), False, 0
        singular = bool(neg & 1) or bad or not np.isfinite(ld)
        return -(ld + ls) / 2, singular

    def form(self, chisq, factor):
        like = self.like
        name = like["form"].lower()
        nm = LD(like.get("nmocks", 1))
        nd = LD(self.N)
        if name == "sellentin":
            return -nm * np.log(1 + chisq / (nm - 1)) / 2 + factor
        if name == "hartlap":
            return -chisq * ((nm - nd - 2) / (nm - 1)) / 2 + factor
        if name == "percival":
            npar = LD(like["nparams"])
            B = (nm - nd - 2) / ((nm - nd - 1) * (nm - nd - 4))
            m = npar + 2 + (nm - 1 + B * (nd - npar)) / (1 + B * (nd - npar))
            return -m * np.log(1 + chisq / (nm - 1)) / 2 + factor
        return -chisq / 2 + factor

    def chi2(self, theory, rows):
        """(lnL, chi2) in longdouble of theory vectors (n, N) at the rows' beta, with the kernels' failure semantics."""
        theory = np.atleast_2d(np.asarray(theory)).astype(LD)
        rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
        lnl = np.empty(len(rows), LD)
        chi = np.empty(len(rows), LD)
        for n, row in enumerate(rows):
            beta = row[N.P_BETA]
            r = theory[n] - self.data_at(beta)
            P, lo, t = self.precision(beta)
            c = r @ P @ r
            factor, singular = self.log_det_factor(lo, t)
            with np.errstate(invalid="ignore", divide="ignore"):
                l = self.form(c, factor)
            if singular or not np.isfinite(t) or np.isnan(l):
                l, c = LD(-np.inf), LD(np.inf)
            lnl[n], chi[n] = l, c
        return lnl, chi

    def log_likelihood(self, rows):
        """(lnL, chi2, theory) of ``rows`` entirely in longdouble."""
        th = self.theory(rows, sens=False).t
        lnl, chi = self.chi2(th, rows)
        return lnl, chi, th


def chi2_from_theory(fit, theory, rows, kw=None, xp=None):
    """chi-square and lnL in longdouble from a given theory matrix (n, N) - the GPU's own theory vectors, so that the
    chi-square kernels are held to the quadratic form alone.  ``fit``: a CCFFit, or a JointFit (blocks' residuals
    concatenated under ONE precision per beta).  Returns (lnl, chi2)."""
    if hasattr(fit, "fits"):
        assert fit.covariance is not None, "a block-diagonal JointFit is a sum of single fits"
        return _joint_chi2(fit, theory, rows)
    xp = xp or XP(fit, kw)
    return xp.chi2(theory, rows)


def _joint_chi2(jf, theory, rows):
    """JointFit with one full covariance: residuals of the blocks concatenated; precision / log det as for one fit on the
    joint covariance grid (victor_amd/joint.py)."""
    theory = np.atleast_2d(np.asarray(theory)).astype(LD)
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    blocks = [XP(f) for f in jf.fits]
    prec = np.asarray(jf.icov, dtype=np.float64).astype(LD)
    fixed = jf.fixed_covmat
    grid = None if fixed else np.asarray(jf.beta_covmat, dtype=np.float64).astype(LD)
    logdet = eig = None
    if not fixed:
        logdet, eig = np.asarray(jf._logdet).astype(LD), np.asarray(jf._eig).astype(LD)
    like = jf.likelihood
    proxy = blocks[0]
    lnl = np.empty(len(rows), LD)
    chi = np.empty(len(rows), LD)
    for n, row in enumerate(rows):
        beta = row[N.P_BETA]
        d = np.concatenate([b.data_at(beta) for b in blocks])
        r = theory[n] - d
        if fixed:
            P, lo, t = prec, 0, LD(0)
        else:
            lo, t = bracket(grid, beta)
            P = prec[lo] if t == 0 or not np.isfinite(t) else (1 - t) * prec[lo] + t * prec[-1]
        c = r @ P @ r
        if fixed:
            factor, singular = LD(0), False
        else:
            if t != 0 and np.isfinite(t):
                fct = (1 - t) + t * eig[lo]
                with np.errstate(divide="ignore", invalid="ignore"):
                    ls = np.log(np.abs(fct)).sum()
                singular = bool(np.sum(fct < 0) & 1) or bool(np.any((fct == 0) | ~np.isfinite(fct)))
            else:
                ls, singular = LD(0), False
            singular = singular or not np.isfinite(logdet[lo])
            factor = -(logdet[lo] + ls) / 2
        proxy.like, proxy.N = like, len(r)
        with np.errstate(invalid="ignore", divide="ignore"):
            l = proxy.form(c, factor)
        if singular or not np.isfinite(t) or np.isnan(l):
            l, c = LD(-np.inf), LD(np.inf)
        lnl[n], chi[n] = l, c
    return lnl, chi
