"""Target distributions -- API of the reference's utils/distributions.py.

Each class keeps the reference's constructor, `get_energy_function()`, `get_samples(n)` and
`log_density(X)`.  The energy function returned is an `EnergyFunction`: calling it on an
(N, d) float32 device tensor evaluates U(x) with the HIP kernel `l2hmc_energy`, and
`Dynamics` reads its `.spec` to fuse U and grad U into the leapfrog kernel (no autograd:
the gradients are analytic, dynamics.py:217-218 used `tf.gradients`).
"""

import numpy as np
import torch

from . import _ffi
from .layers import default_device


class EnergyFunction(object):
    """fn(x, *args, **kwargs) -> (N,) energies, plus the parameters the fused kernels need."""

    def __init__(self, kind, x_dim=None, mu=None, prec=None, logc=None, n_comp=1, eta=0.0,
                 easy=False):
        self.kind, self.x_dim, self.n_comp = kind, x_dim, n_comp
        self.eta, self.easy = float(eta), bool(easy)
        # Rough Well: the reference divides by the Python-double product eps * eps, rounded to float32 once (distributions.py:93)
        self.den = float(np.float32(self.eta if self.easy else self.eta * self.eta)) if kind == _ffi.ENERGY_ROUGHWELL else 0.0
        self._host = {'mu': mu, 'prec': prec, 'logc': logc}
        self._dev = {}

    # -- device-side parameter buffers (built once per device) ---------------------------------
    def _buffers(self, device):
        key = str(device)
        if key not in self._dev:
            L = _ffi.lib()
            buf = {}
            for k in ('mu', 'logc'):
                v = self._host[k]
                buf[k] = None if v is None else torch.as_tensor(
                    np.ascontiguousarray(v, dtype=np.float32), device=device)
            prec = self._host['prec']
            if self.kind == _ffi.ENERGY_GAUSS_DIAG:
                buf['prec'] = torch.as_tensor(np.ascontiguousarray(prec, dtype=np.float32), device=device)
            elif self.kind in (_ffi.ENERGY_GAUSS_DENSE, _ffi.ENERGY_GMM):
                d = self.x_dim
                stride = L.l2hmc_packed_gaussian_floats(d)
                raw = torch.as_tensor(np.ascontiguousarray(prec, dtype=np.float32).reshape(-1, d, d),
                                      device=device)
                packed = torch.empty(raw.shape[0] * stride, dtype=torch.float32, device=device)
                s = _ffi.current_stream(device)
                for i in range(raw.shape[0]):
                    _ffi.check(L.l2hmc_pack_gaussian(raw[i].data_ptr(), d,
                                                     packed.data_ptr() + 4 * i * stride, s))
                buf['prec'], buf['_raw'] = packed, raw
            else:
                buf['prec'] = None
            self._dev[key] = buf
        return self._dev[key]

    def c_struct(self, device, temperature=1.0, anneal_beta=0.0, raw_prec=False):
        """include/l2hmc.h L2hmcEnergy over this device's buffers.  raw_prec: the RAW (k, d, d) precisions of a dense Gaussian /
        mixture instead of their MFMA packing (what the fused training kernels read); the other kinds have one form only."""
        b = self._buffers(device)
        prec = b['_raw'] if raw_prec and '_raw' in b else b['prec']
        return _ffi.L2hmcEnergy(self.kind, self.n_comp, _ffi.ptr(b['mu']), _ffi.ptr(prec),
                                _ffi.ptr(b['logc']), self.eta, int(self.easy), float(temperature),
                                float(anneal_beta), self.den, 0)

    def evaluate(self, x, temperature=1.0, want_U=True, want_grad=False, anneal_beta=0.0):
        x = as_device_f32(x)
        N, d = x.shape
        if self.x_dim is not None and d != self.x_dim:
            raise ValueError("energy expects x_dim=%d, got %d" % (self.x_dim, d))
        U = torch.empty(N, dtype=torch.float32, device=x.device) if want_U else None
        g = torch.empty_like(x) if want_grad else None
        e = self.c_struct(x.device, temperature, anneal_beta)
        _ffi.check(_ffi.lib().l2hmc_energy(e, x.data_ptr(), N, d, _ffi.ptr(U), _ffi.ptr(g),
                                           _ffi.current_stream(x.device)))
        return U, g

    def __call__(self, x, *args, **kwargs):
        return self.evaluate(x)[0]


ENERGY_USER = 100     # python-side tag: a caller-supplied energy (L2hmcSplitArgs.energy_cb)


class UserEnergy(EnergyFunction):
    """A caller-supplied target: ANY callable `fn(x[, aux=...]) -> (N,)` on ROCm tensors that torch can differentiate
    (the `energy_function` protocol of the reference's Dynamics, utils/dynamics.py:203-218: `self._fn(x[, aux])` and
    `tf.gradients` of it) -- e.g. the closure of mnist_vae.py:122-126, or a density that is not in
    utils/distributions.py.  `Dynamics(x_dim, fn)` wraps a plain callable in one of these by itself.

    This is the SLOW path, by construction: U and grad U are computed by the caller's torch code between kernel
    launches (`grad_fn(x[, aux=...]) -> (N, d)` if given, else autograd of `fn`), one host round trip per leapfrog step;
    the leapfrog half-updates, the S/T/Q nets, the log-determinant, the accept probability and the MH select stay on
    the library's HIP kernels (GEMM engine, `l2hmc_trajectory_split`).  Training the sampler on such a target
    (`Trainer(dynamics)`: the GEMM-engine trainer) additionally asks for Hessian-vector products of U, one per leapfrog
    step -- `hvp()` below: double backward through `fn`, or one backward through a differentiable `grad_fn`."""

    def __init__(self, fn, grad_fn=None, x_dim=None):
        EnergyFunction.__init__(self, ENERGY_USER, x_dim=x_dim)
        if not callable(fn) or (grad_fn is not None and not callable(grad_fn)):
            raise TypeError("UserEnergy needs callables")
        self.fn, self.grad_fn = fn, grad_fn

    def _buffers(self, device):
        raise NotImplementedError("a caller-supplied energy has no fused-kernel parameters")

    def c_struct(self, device, temperature=1.0, anneal_beta=0.0, raw_prec=False):
        raise NotImplementedError("a caller-supplied energy runs through L2hmcSplitArgs.energy_cb, not L2hmcEnergy")

    def _call(self, f, x, aux):
        return f(x) if aux is None else f(x, aux=aux)

    def evaluate(self, x, temperature=1.0, want_U=True, want_grad=False, aux=None, anneal_beta=0.0):
        """(U, grad U) of  [(1 - b) |x|^2 / 2 + b] U(x) / temperature  (b = anneal_beta, 0 = off: utils/ais.py:46-47;
        temperature: dynamics.py:203-212) -- U as float64 (the caller's own precision kept as far as it goes)."""
        x = as_device_f32(x)
        U = g = None
        if want_grad and self.grad_fn is None:
            with torch.enable_grad():
                xr = x.clone().requires_grad_(True)
                Ur = self._call(self.fn, xr, aux)
                if Ur.shape != (x.shape[0],):
                    raise ValueError("the energy function must return shape (N,), got %s" % (tuple(Ur.shape),))
                g, = torch.autograd.grad(Ur.sum(), xr)         # dynamics.py:217-218: tf.gradients sums over the batch
            U = Ur.detach()
        else:
            with torch.no_grad():
                if want_U:
                    U = self._call(self.fn, x, aux)
                    if U.shape != (x.shape[0],):
                        raise ValueError("the energy function must return shape (N,), got %s" % (tuple(U.shape),))
                if want_grad:
                    g = self._call(self.grad_fn, x, aux)
        b = float(anneal_beta)
        if b > 0.0 and b != 1.0:
            if U is not None:
                U = (1.0 - b) * 0.5 * x.double().square().sum(1) + b * U.double()
            if g is not None:
                g = (1.0 - b) * x + b * g
        if temperature != 1.0:
            U = None if U is None else U.double() / float(temperature)
            g = None if g is None else g / float(temperature)
        return (U.double() if (U is not None and want_U) else None), (g.to(torch.float32) if g is not None else None)

    def hvp(self, x, u, aux=None):
        """(d^2 U / dx^2)(x) u, shape (N, d): what the training loss needs where it back-propagates through grad U
        (utils/dynamics.py:218 inside the differentiated graph)."""
        x, u = as_device_f32(x), as_device_f32(u)
        with torch.enable_grad():
            xr = x.clone().requires_grad_(True)
            if self.grad_fn is None:
                Ur = self._call(self.fn, xr, aux)
                g, = torch.autograd.grad(Ur.sum(), xr, create_graph=True)
            else:
                g = self._call(self.grad_fn, xr, aux)
                if not g.requires_grad:
                    raise NotImplementedError("training needs Hessian-vector products: grad_energy must be torch code "
                                              "that autograd can differentiate (or leave it out and pass a differentiable "
                                              "energy function)")
            hv, = torch.autograd.grad((g * u).sum(), xr)
        return hv.to(torch.float32)

    def __call__(self, x, aux=None, *args, **kwargs):
        return self.evaluate(x, aux=aux)[0].to(torch.float32)


class LogisticEnergy(EnergyFunction):
    """U(w) = sum_i [softplus(x_i . w) - y_i x_i . w] + |w|^2 / (2 prior_var) on the fused kernels (L2HMC_ENERGY_LOGISTIC): the
    data set is packed into the kernels' fragment order once per device (`l2hmc_pack_logistic`)."""

    def __init__(self, X, y, prior_var):
        n, d = X.shape
        EnergyFunction.__init__(self, _ffi.ENERGY_LOGISTIC, d, n_comp=n, eta=prior_var)
        self._host = {'X': X, 'y': y}

    def _buffers(self, device):
        key = str(device)
        if key not in self._dev:
            L = _ffi.lib()
            X = torch.as_tensor(self._host['X'], device=device)
            y = torch.as_tensor(self._host['y'], device=device)
            n, d = X.shape
            packed = torch.empty(_ffi.check(L.l2hmc_packed_logistic_floats(n, d)), dtype=torch.float32, device=device)
            _ffi.check(L.l2hmc_pack_logistic(X.data_ptr(), y.data_ptr(), n, d, packed.data_ptr(), _ffi.current_stream(device)))
            self._dev[key] = {'mu': packed, 'prec': None, 'logc': None, '_X': X, '_y': y}
        return self._dev[key]


class PoissonEnergy(EnergyFunction):
    """U(w) = sum_i [exp(h_i) - y_i h_i] + |w|^2 / (2 prior_var), h_i = x_i . w + offset_i, on the fused kernels
    (L2HMC_ENERGY_POISSON): the data set is packed once per device into the buffer `LogisticEnergy` uses, the counts in its
    label slot (`l2hmc_pack_logistic`: what `glm.Glm` packs for the history statistics), and the offsets go beside it, zero-padded
    to whole 16-row blocks (`l2hmc_poisson_offset_floats`; L2hmcEnergy.prec)."""

    def __init__(self, X, y, offset, prior_var):
        n, d = X.shape
        EnergyFunction.__init__(self, _ffi.ENERGY_POISSON, d, n_comp=n, eta=prior_var)
        self._host = {'X': X, 'y': y, 'offset': np.zeros(n, dtype=np.float32) if offset is None else offset}

    def _buffers(self, device):
        key = str(device)
        if key not in self._dev:
            L = _ffi.lib()
            X = torch.as_tensor(np.ascontiguousarray(self._host['X'], dtype=np.float32), device=device)
            y = torch.as_tensor(np.ascontiguousarray(self._host['y'], dtype=np.float32), device=device)
            n, d = X.shape
            packed = torch.empty(_ffi.check(L.l2hmc_packed_logistic_floats(n, d)), dtype=torch.float32, device=device)
            _ffi.check(L.l2hmc_pack_logistic(X.data_ptr(), y.data_ptr(), n, d, packed.data_ptr(), _ffi.current_stream(device)))
            off = torch.zeros(_ffi.check(L.l2hmc_poisson_offset_floats(n)), dtype=torch.float32, device=device)
            off[:n] = torch.as_tensor(np.ascontiguousarray(self._host['offset'], dtype=np.float32), device=device)
            self._dev[key] = {'mu': packed, 'prec': off, 'logc': None, '_X': X, '_y': y}
        return self._dev[key]


class BinomialEnergy(EnergyFunction):
    """U(w) = sum_i [m_i softplus(t_i) - y_i t_i] + |w|^2 / (2 prior_var), t_i = x_i . w + o_i, on the fused kernels
    (L2HMC_ENERGY_BINOMIAL): binomial regression (m = trials, o = offset) and negative-binomial regression with fixed
    dispersion (m = y + phi, o = offset - log phi).  The data set is packed once per device into the buffer `LogisticEnergy`
    uses, y in its label slot, and the row constants go beside it: per 16-row block [16 offsets | 16 weights], zero-padded
    (`l2hmc_binomial_aux_floats`; L2hmcEnergy.prec)."""

    KIND = _ffi.ENERGY_BINOMIAL

    def __init__(self, X, y, offset, weight, prior_var):
        n, d = X.shape
        EnergyFunction.__init__(self, self.KIND, d, n_comp=n, eta=prior_var)
        self._host = {'X': X, 'y': y, 'offset': offset, 'weight': weight}

    def _buffers(self, device):
        key = str(device)
        if key not in self._dev:
            L = _ffi.lib()
            X = torch.as_tensor(np.ascontiguousarray(self._host['X'], dtype=np.float32), device=device)
            y = torch.as_tensor(np.ascontiguousarray(self._host['y'], dtype=np.float32), device=device)
            n, d = X.shape
            packed = torch.empty(_ffi.check(L.l2hmc_packed_logistic_floats(n, d)), dtype=torch.float32, device=device)
            _ffi.check(L.l2hmc_pack_logistic(X.data_ptr(), y.data_ptr(), n, d, packed.data_ptr(), _ffi.current_stream(device)))
            floats = _ffi.check(L.l2hmc_binomial_aux_floats(n))
            aux = np.zeros((floats // 32, 2, 16), dtype=np.float32)
            for k, name in enumerate(('offset', 'weight')):
                rows = np.zeros(16 * (floats // 32), dtype=np.float32)
                rows[:n] = self._host[name]
                aux[:, k, :] = rows.reshape(-1, 16)
            self._dev[key] = {'mu': packed, 'prec': torch.as_tensor(aux.reshape(-1), device=device), 'logc': None, '_X': X, '_y': y}
        return self._dev[key]


class ProbitEnergy(BinomialEnergy):
    """U(w) = -sum_i [y_i log Phi(t_i) + (m_i - y_i) log Phi(-t_i)] + |w|^2 / (2 prior_var), t_i = x_i . w + o_i, on the fused
    kernels (L2HMC_ENERGY_PROBIT): `BinomialEnergy`'s buffers -- the packed data and the [16 offsets | 16 trials] blocks -- under
    the probit link's kind."""
    KIND = _ffi.ENERGY_PROBIT


class LogisticRegression(object):
    """Bayesian logistic regression: labels y_i in {0, 1} with P(y_i = 1 | w) = sigmoid(x_i . w) and a N(0, prior_var I) prior
    on the weights w (d = X.shape[1] <= 128 features; add a column of ones for an intercept).  The posterior's energy

        U(w) = sum_i [softplus(x_i . w) - y_i x_i . w] + |w|^2 / (2 prior_var)

    and its gradient X^T (sigmoid(X w) - y) + w / prior_var are fused into the trajectory kernels (two f32 MFMA contractions
    over the data per gradient): HMC and L2HMC sampling, parallel tempering and AIS run on it like on any built-in target.
    A sampler trains on it with `LogisticTrainer` (the tile training kernel's logistic-regression form: the Hessian-vector
    product is one more contraction over the data); shapes beyond that kernel's LDS plan train on the same likelihood written
    as a torch callable."""

    def __init__(self, X, y, prior_var=1.0):
        X = np.asarray(X, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
            raise ValueError("X must be (n_data, d) with n_data, d >= 1, got shape %s" % (X.shape,))
        n, d = X.shape
        if d > 128:
            raise ValueError("LogisticRegression supports d <= 128 features (got %d)" % d)
        if n > 1 << 20:
            raise ValueError("LogisticRegression supports at most 1048576 data rows (got %d)" % n)
        if y.shape != (n,):
            raise ValueError("y must be (n_data,) = (%d,), got shape %s" % (n, y.shape))
        if not np.all(np.isfinite(X)):
            raise ValueError("X must be finite")
        if not np.all((y == 0.0) | (y == 1.0)):
            raise ValueError("labels y must be 0 or 1")
        prior_var = float(prior_var)
        if not (np.isfinite(prior_var) and prior_var > 0.0):
            raise ValueError("prior_var must be finite and > 0, got %r" % (prior_var,))
        self.X = np.ascontiguousarray(X, dtype=np.float32)
        self.y = np.ascontiguousarray(y, dtype=np.float32)
        self.prior_var = prior_var
        self.dim = d

    def get_energy_function(self):
        return LogisticEnergy(self.X, self.y, self.prior_var)

    def log_density(self, W):
        """Unnormalised log posterior -U(w) of each row of W (n_w, d), in float64."""
        W = np.asarray(W, dtype=np.float64)
        L = W @ self.X.astype(np.float64).T
        nll = np.logaddexp(0.0, L) - L * self.y.astype(np.float64)
        return -(nll.sum(axis=1) + 0.5 * np.square(W).sum(axis=1) / self.prior_var)

    def predict_proba(self, draws, X=None):
        """The posterior predictive P(y = 1) of every row of X (default: the model's own rows) under the draws -- a recorded
        history (M, N, d) or a matrix (S, d); a ROCm tensor is read where it lies (`predictive.predict_proba`)."""
        from . import predictive
        return predictive.predict_proba(draws, self.X if X is None else X)

    def waic(self, draws):
        """WAIC of this model's own data under the draws (`predictive.waic`): a `Summary` with elpd_waic, p_waic, lppd, se."""
        from . import predictive
        return predictive.waic(draws, self.X, self.y)

    def loo(self, draws, finish="torch", r_eff=None):
        """PSIS-LOO of this model's own data under the draws (`predictive.loo`): a `Summary` with elpd_loo, p_loo, looic, se,
        the per-row Pareto `khat` and `n_bad`, the number of rows where it exceeds 0.7.  `finish="kernel"`: the Pareto fit on
        the fused kernels of csrc/psis.hip (device draws only).  `r_eff="auto"` (or an array): tail lengths, `n_eff` and
        `mcse_elpd_loo` for autocorrelated draws (`predictive.loo`)."""
        from . import predictive
        return predictive.loo(draws, self.X, self.y, finish=finish, r_eff=r_eff)

    def relative_eff(self, draws, max_lag=None, split=False):
        """The per-row relative efficiency r_eff_i = ESS(P(y_i | x_i, w)) / S of this model's own data under a recorded history
        (steps, chains, dim) (`predictive.relative_eff`): a `Summary` with r_eff, ess, truncated, n_nan."""
        from . import predictive
        return predictive.relative_eff(draws, self.X, self.y, max_lag=max_lag, split=split)


class PoissonRegression(object):
    """Bayesian Poisson regression with the log link: counts y_i ~ Poisson(exp(x_i . w + offset_i)) (offset = log exposure,
    default 0) and a N(0, prior_var I) prior on the weights w (d <= 128 features).  The posterior's energy

        U(w) = sum_i [exp(x_i . w + o_i) - y_i (x_i . w + o_i)] + |w|^2 / (2 prior_var)

    and its gradient X^T (mu - y) + w / prior_var exist in two forms.  `get_energy_function(fused=True)` is a `PoissonEnergy`:
    U and grad U fused into the general trajectory kernel (L2HMC_ENERGY_POISSON: the two f32 MFMA contractions over the packed
    data of the logistic-regression target with the log link between them), so HMC and L2HMC sampling, `warmup`, parallel
    tempering and AIS run on it like on any built-in target; exp overflows as float32 does, and a proposal whose energy is
    not finite is rejected.  `get_energy_function()` -- the default -- is a `UserEnergy` with the same gradient as
    differentiable torch code: the slow path (one host round trip per leapfrog step), and the one a sampler TRAINS on, since
    no training kernel holds the Hessian-vector product X^T [mu (X u)]: `Trainer(dynamics)` on the slow-path energy, then
    `load_state_dict` into a `Dynamics` on the fused one.  Everything computed FROM the recorded history is fused HIP
    (csrc/glm.hip; `l2hmc_amd.glm`): the predictive mean, WAIC and PSIS-LOO never form the (draws, rows) log-likelihood matrix,
    and they evaluate mu by the very float32 operations the fused energy uses."""

    def __init__(self, X, y, offset=None, prior_var=1.0):
        from . import glm
        X = np.asarray(X, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
            raise ValueError("X must be (n_data, d) with n_data, d >= 1, got shape %s" % (X.shape,))
        n, d = X.shape
        if d > 128:
            raise ValueError("PoissonRegression supports d <= 128 features (got %d)" % d)
        if n > 1 << 20:
            raise ValueError("PoissonRegression supports at most 1048576 data rows (got %d)" % n)
        if y.shape != (n,):
            raise ValueError("y must be (n_data,) = (%d,), got shape %s" % (n, y.shape))
        if not np.all(np.isfinite(X)):
            raise ValueError("X must be finite")
        if not np.all(np.isfinite(y)) or not np.all((y >= 0.0) & (y == np.floor(y)) & (y <= glm.MAX_COUNT)):
            raise ValueError("counts y must be non-negative integers <= 2^24")
        offset = np.zeros(n) if offset is None else np.asarray(offset, dtype=np.float64)
        if offset.shape != (n,) or not np.all(np.isfinite(offset)):
            raise ValueError("offset must be finite (n_data,) = (%d,), got shape %s" % (n, offset.shape))
        prior_var = float(prior_var)
        if not (np.isfinite(prior_var) and prior_var > 0.0):
            raise ValueError("prior_var must be finite and > 0, got %r" % (prior_var,))
        self.X = np.ascontiguousarray(X, dtype=np.float32)
        self.y = np.ascontiguousarray(y, dtype=np.float32)
        self.offset = np.ascontiguousarray(offset, dtype=np.float32)
        self.prior_var = prior_var
        self.dim = d
        self._glm = glm.Glm(self.X, self.y, self.offset)
        self._torch = {}

    def _data(self, x):
        key = (str(x.device), x.dtype)
        if key not in self._torch:
            self._torch[key] = tuple(torch.as_tensor(a).to(device=x.device, dtype=x.dtype) for a in (self.X, self.y, self.offset))
        return self._torch[key]

    def energy(self, x):
        """U(w) of each row of the torch tensor x (N, d), in x's own device and dtype; differentiable."""
        X, y, o = self._data(x)
        h = x @ X.t() + o
        return (torch.exp(h) - y * h).sum(dim=1) + 0.5 * x.square().sum(dim=1) / self.prior_var

    def grad_energy(self, x):
        """grad U = X^T (mu - y) + w / prior_var, (N, d); differentiable (the trainer's Hessian-vector products)."""
        X, y, o = self._data(x)
        return (torch.exp(x @ X.t() + o) - y) @ X + x / self.prior_var

    def get_energy_function(self, fused=False):
        """The posterior's energy: a `UserEnergy` (torch code, the slow path; what `Trainer` takes), or with `fused=True` a
        `PoissonEnergy` on the fused trajectory kernels (sampling, warm-up, tempering, AIS)."""
        if fused:
            return PoissonEnergy(self.X, self.y, self.offset, self.prior_var)
        return UserEnergy(self.energy, self.grad_energy, x_dim=self.dim)

    def log_density(self, W):
        """Unnormalised log posterior -U(w) of each row of W (n_w, d), in float64."""
        W = np.asarray(W, dtype=np.float64)
        h = W @ self.X.astype(np.float64).T + self.offset.astype(np.float64)
        return -((np.exp(h) - self.y.astype(np.float64) * h).sum(axis=1) + 0.5 * np.square(W).sum(axis=1) / self.prior_var)

    def log_lik(self, draws, rows=None):
        """The pointwise log-likelihood matrix (S, m) of a range of rows (`glm.Glm.log_lik`): the slow route."""
        return self._glm.log_lik(draws, rows=rows)

    def predict_mean(self, draws, X=None, offset=None):
        """The posterior predictive mean of every row of X (default: the model's own rows) under the draws."""
        return self._glm.predict_mean(draws, X=X, offset=offset)

    def waic(self, draws):
        """WAIC of this model's own data under the draws: a `Summary` with elpd_waic, p_waic, lppd, se, elpd_i,
        n_high_variance, n_underflow."""
        return self._glm.waic(draws)

    def loo(self, draws, r_eff=None, max_lag=None, split=False, max_tail_bytes=256 << 20):
        """PSIS-LOO of this model's own data under the draws (`glm.Glm.loo`): the fields of `loo_from_log_lik`."""
        return self._glm.loo(draws, r_eff=r_eff, max_lag=max_lag, split=split, max_tail_bytes=max_tail_bytes)

    def relative_eff(self, draws, max_lag=None, split=False, max_bytes=256 << 20):
        """The per-row relative efficiency of this model's own data under a recorded history (`glm.Glm.relative_eff`)."""
        return self._glm.relative_eff(draws, max_lag=max_lag, split=split, max_bytes=max_bytes)


class _WeightedLogitRegression(object):
    """What `BinomialRegression` and `NegativeBinomialRegression` share (and `ProbitRegression`, which keeps the data handling,
    the row constants and the statistics and overrides the energy with the probit link's): one likelihood (include/l2hmc.h, L2HMC_ENERGY_BINOMIAL)

        ll_i = y_i t_i - m_i softplus(t_i) + c_i,   t_i = x_i . w + o_i,    U(w) = sum_i [m_i softplus(t_i) - y_i t_i] + |w|^2 / (2 prior_var)

    with per-row constants (o, m, c) that the subclass's family forms in float64 (`glm.Binomial`, `glm.NegBinomial`) and that
    are rounded to float32 once.  `get_energy_function(fused=True)` is a `BinomialEnergy`: U and grad U = X^T (m sigmoid(t) - y)
    + w / prior_var fused into the general trajectory kernel, so HMC and L2HMC sampling, `warmup`, parallel tempering and AIS
    run on it like on any built-in target; nothing in it can overflow.  `get_energy_function()` -- the default -- is a
    `UserEnergy` with the same gradient as differentiable torch code: the slow path, and the one a sampler TRAINS on (no
    training kernel holds the Hessian-vector product X^T [m s (1 - s) (X u)]): `Trainer(dynamics)` on the slow-path energy,
    then `load_state_dict` into a `Dynamics` on the fused one.  Everything computed FROM the recorded history is fused HIP
    (csrc/glm.hip; `l2hmc_amd.glm`) and evaluates t and softplus by the very float32 operations the fused energy uses.  A
    float32 ll loses absolute accuracy in proportion to m |t|."""

    _name = None
    _fused = BinomialEnergy

    def _init(self, X, y, offset, prior_var, family, weight, check_y):
        from . import glm
        X = np.asarray(X, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
            raise ValueError("X must be (n_data, d) with n_data, d >= 1, got shape %s" % (X.shape,))
        n, d = X.shape
        if d > 128:
            raise ValueError("%s supports d <= 128 features (got %d)" % (self._name, d))
        if n > 1 << 20:
            raise ValueError("%s supports at most 1048576 data rows (got %d)" % (self._name, n))
        if y.shape != (n,):
            raise ValueError("y must be (n_data,) = (%d,), got shape %s" % (n, y.shape))
        if not np.all(np.isfinite(X)):
            raise ValueError("X must be finite")
        weight = check_y(y, n)
        offset = np.zeros(n) if offset is None else np.asarray(offset, dtype=np.float64)
        if offset.shape != (n,) or not np.all(np.isfinite(offset)):
            raise ValueError("offset must be finite (n_data,) = (%d,), got shape %s" % (n, offset.shape))
        prior_var = float(prior_var)
        if not (np.isfinite(prior_var) and prior_var > 0.0):
            raise ValueError("prior_var must be finite and > 0, got %r" % (prior_var,))
        self.X = np.ascontiguousarray(X, dtype=np.float32)
        self.y = np.ascontiguousarray(y, dtype=np.float32)
        self.offset = np.ascontiguousarray(offset, dtype=np.float32)
        self.prior_var = prior_var
        self.dim = d
        self._glm = glm.Glm(self.X, self.y, self.offset, family, None if weight is None else np.ascontiguousarray(weight, dtype=np.float32))
        self._o, self._m = self._glm.consts[0], self._glm.consts[1]      # the float32 (o, m) of the likelihood: the kernels' own
        self._torch = {}

    def _data(self, x):
        key = (str(x.device), x.dtype)
        if key not in self._torch:
            self._torch[key] = tuple(torch.as_tensor(a).to(device=x.device, dtype=x.dtype) for a in (self.X, self.y, self._o, self._m))
        return self._torch[key]

    def energy(self, x):
        """U(w) of each row of the torch tensor x (N, d), in x's own device and dtype; differentiable."""
        X, y, o, m = self._data(x)
        t = x @ X.t() + o
        return (m * torch.nn.functional.softplus(t) - y * t).sum(dim=1) + 0.5 * x.square().sum(dim=1) / self.prior_var

    def grad_energy(self, x):
        """grad U = X^T (m sigmoid(t) - y) + w / prior_var, (N, d); differentiable (the trainer's Hessian-vector products)."""
        X, y, o, m = self._data(x)
        return (m * torch.sigmoid(x @ X.t() + o) - y) @ X + x / self.prior_var

    def get_energy_function(self, fused=False):
        """The posterior's energy: a `UserEnergy` (torch code, the slow path; what `Trainer` takes), or with `fused=True` a
        `BinomialEnergy` on the fused trajectory kernels (sampling, warm-up, tempering, AIS)."""
        if fused:
            return self._fused(self.X, self.y, self._o, self._m, self.prior_var)
        return UserEnergy(self.energy, self.grad_energy, x_dim=self.dim)

    def log_density(self, W):
        """Unnormalised log posterior -U(w) of each row of W (n_w, d), in float64 (the constants c_i are not part of U)."""
        W = np.asarray(W, dtype=np.float64)
        o, m, _ = self._glm.lik.terms(self.y, self.offset, self._glm.weight)
        t = W @ self.X.astype(np.float64).T + o
        return -((m * np.logaddexp(0.0, t) - self.y.astype(np.float64) * t).sum(axis=1) + 0.5 * np.square(W).sum(axis=1) / self.prior_var)

    def log_lik(self, draws, rows=None):
        """The pointwise log-likelihood matrix (S, m) of a range of rows (`glm.Glm.log_lik`): the slow route."""
        return self._glm.log_lik(draws, rows=rows)

    def waic(self, draws):
        """WAIC of this model's own data under the draws: a `Summary` with elpd_waic, p_waic, lppd, se, elpd_i,
        n_high_variance, n_underflow."""
        return self._glm.waic(draws)

    def loo(self, draws, r_eff=None, max_lag=None, split=False, max_tail_bytes=256 << 20):
        """PSIS-LOO of this model's own data under the draws (`glm.Glm.loo`): the fields of `loo_from_log_lik`."""
        return self._glm.loo(draws, r_eff=r_eff, max_lag=max_lag, split=split, max_tail_bytes=max_tail_bytes)

    def relative_eff(self, draws, max_lag=None, split=False, max_bytes=256 << 20):
        """The per-row relative efficiency of this model's own data under a recorded history (`glm.Glm.relative_eff`)."""
        return self._glm.relative_eff(draws, max_lag=max_lag, split=split, max_bytes=max_bytes)


class BinomialRegression(_WeightedLogitRegression):
    """Bayesian binomial regression with the logit link: y_i successes out of trials_i ~ Binomial(trials_i, sigmoid(x_i . w +
    offset_i)) and a N(0, prior_var I) prior on the weights w (d <= 128 features) -- aggregated binary data without one row
    per trial.  `trials`: integers with 1 <= trials <= 2^24 and 0 <= y <= trials; a scalar broadcasts.  trials = 1 is
    `LogisticRegression`'s posterior."""

    _name = "BinomialRegression"

    def __init__(self, X, y, trials, offset=None, prior_var=1.0):
        from . import glm
        self._check_and_init(X, y, trials, offset, prior_var, glm.Binomial())

    def _check_and_init(self, X, y, trials, offset, prior_var, family):
        """The checks of y against `trials` and the shared `_init` under `family` (`ProbitRegression` calls it too)."""
        from . import glm

        def check_y(y, n):
            m = np.asarray(trials, dtype=np.float64)
            if m.ndim == 0:
                m = np.full(n, float(m))
            if m.shape != (n,):
                raise ValueError("trials must be a scalar or (n_data,) = (%d,), got shape %s" % (n, m.shape))
            if not np.all(np.isfinite(m)) or not np.all((m >= 1.0) & (m == np.floor(m)) & (m <= glm.MAX_COUNT)):
                raise ValueError("trials must be integers with 1 <= trials <= 2^24")
            if not np.all(np.isfinite(y)) or not np.all((y >= 0.0) & (y == np.floor(y)) & (y <= m)):
                raise ValueError("successes y must be integers with 0 <= y <= trials")
            return m
        self._init(X, y, offset, prior_var, family, None, check_y)
        self.trials = self._glm.weight

    def predict_mean(self, draws, X=None, offset=None, trials=None):
        """The posterior predictive mean E[y | x] = trials x mean over the draws of sigmoid(x . w + offset) of every row of X
        (default: the model's own rows, offsets and trials; new rows take `offset`, default 0, and `trials`, default 1: the
        success probability)."""
        return self._glm.predict_mean(draws, X=X, offset=offset, weight=trials)


class ProbitRegression(_WeightedLogitRegression):
    """Bayesian binomial regression with the PROBIT link: y_i successes out of trials_i ~ Binomial(trials_i, Phi(x_i . w +
    offset_i)), Phi the standard normal distribution function, and a N(0, prior_var I) prior on the weights w (d <= 128
    features).  `trials` as `BinomialRegression`'s (default 1: binary probit regression).  With t = x . w + o and
    lam(t) = phi(t) / Phi(t),

        ll_i = y_i log Phi(t_i) + (m_i - y_i) log Phi(-t_i) + log C(m_i, y_i),    U(w) = -sum_i (ll_i - log C) + |w|^2 / (2 prior_var),
        grad U = X^T ((m - y) lam(-t) - y lam(t)) + w / prior_var.

    It shares the data handling, the row constants and the history statistics of `BinomialRegression` (the base class keeps
    its name; only the link between the two data contractions differs): `get_energy_function(fused=True)` is a `ProbitEnergy`
    (L2HMC_ENERGY_PROBIT) on the general trajectory kernel -- sampling, `warmup`, parallel tempering, AIS -- and `log_lik`,
    `predict_mean`, `waic`, `loo` and `relative_eff` of a recorded history run on csrc/glm.hip's kernels (L2HMC_GLM_PROBIT),
    which evaluate log Phi by the very float32 operations the fused energy uses: one erfcx, accurate in both tails, so a row
    at t = -30 has ll = -454 and not -inf.  `get_energy_function()` -- the default -- is the slow path, a `UserEnergy` in
    differentiable torch code (`torch.special.log_ndtr`) with the analytic gradient: what a sampler TRAINS on (no training
    kernel holds this link), then `load_state_dict` into a `Dynamics` on the fused energy."""

    _name = "ProbitRegression"
    _fused = ProbitEnergy
    _LOG_SQRT_2PI = 0.9189385332046727

    def __init__(self, X, y, trials=1, offset=None, prior_var=1.0):
        from . import glm
        BinomialRegression._check_and_init(self, X, y, trials, offset, prior_var, glm.Probit())

    def _lam(self, t):
        """phi(t) / Phi(t) = exp(-t^2 / 2 - log sqrt(2 pi) - log Phi(t)): finite in both tails, differentiable."""
        return torch.exp(-0.5 * t * t - self._LOG_SQRT_2PI - torch.special.log_ndtr(t))

    def energy(self, x):
        """U(w) of each row of the torch tensor x (N, d), in x's own device and dtype; differentiable."""
        X, y, o, m = self._data(x)
        t = x @ X.t() + o
        nll = -(y * torch.special.log_ndtr(t) + (m - y) * torch.special.log_ndtr(-t))
        return nll.sum(dim=1) + 0.5 * x.square().sum(dim=1) / self.prior_var

    def grad_energy(self, x):
        """grad U = X^T ((m - y) lam(-t) - y lam(t)) + w / prior_var, (N, d); differentiable (the trainer's Hessian-vector
        products)."""
        X, y, o, m = self._data(x)
        t = x @ X.t() + o
        return ((m - y) * self._lam(-t) - y * self._lam(t)) @ X + x / self.prior_var

    def log_density(self, W):
        """Unnormalised log posterior -U(w) of each row of W (n_w, d), in float64 (the constants c_i are not part of U)."""
        W = np.asarray(W, dtype=np.float64)
        lik = self._glm.lik
        o, m, _ = lik.terms(self.y, self.offset, self._glm.weight)
        y = self.y.astype(np.float64)
        t = W @ self.X.astype(np.float64).T + o
        return (y * lik.log_ndtr(t) + (m - y) * lik.log_ndtr(-t)).sum(axis=1) - 0.5 * np.square(W).sum(axis=1) / self.prior_var

    def predict_mean(self, draws, X=None, offset=None, trials=None):
        """The posterior predictive mean E[y | x] = trials x mean over the draws of Phi(x . w + offset) of every row of X
        (default: the model's own rows, offsets and trials; new rows take `offset`, default 0, and `trials`, default 1: the
        success probability)."""
        return self._glm.predict_mean(draws, X=X, offset=offset, weight=trials)


class NegativeBinomialRegression(_WeightedLogitRegression):
    """Bayesian negative-binomial regression (NB2) with the log link: counts y_i with mean mu_i = exp(x_i . w + offset_i) and
    variance mu_i + mu_i^2 / dispersion, the dispersion phi a fixed finite scalar > 0 (not sampled), and a N(0, prior_var I)
    prior on the weights w (d <= 128 features; counts <= 2^24) -- the overdispersed alternative to `PoissonRegression`, which
    it approaches as phi grows; compare the two by `loo`."""

    _name = "NegativeBinomialRegression"

    def __init__(self, X, y, dispersion, offset=None, prior_var=1.0):
        from . import glm
        phi = float(dispersion)
        if not (np.isfinite(phi) and phi > 0.0):
            raise ValueError("dispersion must be finite and > 0, got %r" % (dispersion,))

        def check_y(y, n):
            if not np.all(np.isfinite(y)) or not np.all((y >= 0.0) & (y == np.floor(y)) & (y <= glm.MAX_COUNT)):
                raise ValueError("counts y must be non-negative integers <= 2^24")
            return None
        self._init(X, y, offset, prior_var, glm.NegBinomial(phi), None, check_y)
        self.dispersion = phi

    def predict_mean(self, draws, X=None, offset=None):
        """The posterior predictive mean of every row of X (default: the model's own rows) under the draws."""
        return self._glm.predict_mean(draws, X=X, offset=offset)


def as_device_f32(x, device=None):
    """numpy / torch input -> contiguous float32 tensor on the GPU."""
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(np.asarray(x, dtype=np.float32), device=device or default_device())
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.to(torch.float32).contiguous()
    if not x.is_cuda:
        raise RuntimeError("l2hmc_amd: tensors must live on a ROCm device (got %s); "
                           "there is no CPU path" % x.device)
    return x.detach()


def _rng(rng):
    """Samplers take an optional numpy RandomState; default = numpy's global stream (what the
    reference uses everywhere)."""
    return np.random if rng is None else rng


def _log_spaced_spectrum(dim, log_min, log_max, jitter, rng=None):
    """Random rotation R and eigenvalues 10**U(log_min, log_max) (+ jitter) of a tilted Gaussian."""
    from scipy.stats import ortho_group
    R = ortho_group.rvs(dim)
    eig = 10.0 ** _rng(rng).uniform(log_min, log_max, size=dim) + jitter
    return R, eig


def quadratic_gaussian(x, mu, S):
    """Row-wise 0.5 (x - mu)^T S (x - mu)  (distributions.py:31-32; the reference forms the
    whole N x N product and keeps its diagonal -- only the diagonal is computed here)."""
    S = np.asarray(S, dtype=np.float32)
    return EnergyFunction(_ffi.ENERGY_GAUSS_DENSE, S.shape[0], mu=np.asarray(mu), prec=S)(x)


class Gaussian(object):
    """N(mu, sigma)  (distributions.py:41-68).  The precision is inverted in float64 and used
    in float32, like the reference (:48,52)."""

    def __init__(self, mu, sigma):
        self.mu = np.asarray(mu)
        self.sigma = np.asarray(sigma)
        self.i_sigma = np.linalg.inv(self.sigma.copy())

    def get_energy_function(self):
        S = self.i_sigma.astype(np.float32)
        mu = self.mu.astype(np.float32)
        d = S.shape[0]
        off_diag = S[~np.eye(d, dtype=bool)]
        if d > 1 and not off_diag.any():              # exactly diagonal precision: elementwise path
            return EnergyFunction(_ffi.ENERGY_GAUSS_DIAG, d, mu=mu, prec=np.diag(S).copy())
        return EnergyFunction(_ffi.ENERGY_GAUSS_DENSE, d, mu=mu, prec=S)

    def get_samples(self, n, rng=None):
        """Exact draws mu + L z, L = chol(sigma).  (The reference omits mu; its targets are
        centred, so the two agree there.)"""
        L = np.linalg.cholesky(self.sigma)
        z = _rng(rng).randn(n, L.shape[0])
        return self.mu + z @ L.T

    def log_density(self, X):
        from scipy.stats import multivariate_normal
        return multivariate_normal(mean=self.mu, cov=self.sigma).logpdf(X)


def random_tilted_gaussian(dim, log_min=-2., log_max=2.):
    """Zero-mean Gaussian with a random rotation and log-uniform spectrum (distributions.py:34-39)."""
    R, eig = _log_spaced_spectrum(dim, log_min, log_max, 1e-6)
    return Gaussian(np.zeros(dim), (R.T * eig) @ R)


class TiltedGaussian(Gaussian):
    """distributions.py:70-82; `get_samples(n)` honours n (the reference always drew 200)."""

    def __init__(self, dim, log_min, log_max):
        self.dim = dim
        self.R, eig = _log_spaced_spectrum(dim, log_min, log_max, 1e-8)
        self.diag = np.diag(eig)
        Gaussian.__init__(self, np.zeros(dim), (self.R.T * eig) @ self.R)

    def get_samples(self, n, rng=None):
        z = _rng(rng).randn(n, self.dim)
        return (z * np.sqrt(np.diag(self.diag))) @ self.R


class RoughWell(object):
    """U(x) = |x|^2 / 2 + eps sum_k cos(x_k / eps^2)  (x_k / eps when `easy`)  -- distributions.py:84-101."""

    def __init__(self, dim, eps, easy=False):
        self.dim, self.eps, self.easy = dim, eps, easy

    def get_energy_function(self):
        return EnergyFunction(_ffi.ENERGY_ROUGHWELL, self.dim, eta=self.eps, easy=self.easy)

    def get_samples(self, n, rng=None):
        # for small eps the well is a standard normal to a good approximation (:99-101)
        return _rng(rng).randn(n, self.dim)


class GMM(object):
    """Mixture of Gaussians  (distributions.py:104-152).  Per component the reference keeps
    inv(sigma_i) and c_i = pi_i / sqrt((2 pi)^k det sigma_i) as float32 (:117-124)."""

    def __init__(self, mus, sigmas, pis):
        if len(mus) != len(sigmas) or len(mus) != len(pis):
            raise ValueError("mus, sigmas, pis must have one entry per component")
        if sum(pis) != 1.0:
            raise ValueError("mixture weights must sum to 1")
        self.mus, self.sigmas, self.pis = mus, sigmas, pis
        self.nb_mixtures = len(pis)
        self.k = int(np.asarray(mus[0]).shape[0])
        two_pi_k = (2 * np.pi) ** self.k
        self.i_sigmas = [np.linalg.inv(sg).astype(np.float32) for sg in sigmas]
        norms = [np.float32(np.sqrt(two_pi_k * np.linalg.det(sg))) for sg in sigmas]
        self.constants = [np.float32(pi / nz) for pi, nz in zip(pis, norms)]

    def get_energy_function(self):
        return EnergyFunction(_ffi.ENERGY_GMM, self.k,
                              mu=np.stack([np.asarray(m, dtype=np.float32) for m in self.mus]),
                              prec=np.stack(self.i_sigmas),
                              logc=np.log(np.asarray(self.constants, dtype=np.float32)),
                              n_comp=self.nb_mixtures)

    def get_samples(self, n, rng=None):
        r = _rng(rng)
        comp = r.choice(self.nb_mixtures, size=n, p=self.pis)
        out = np.empty((n, self.k))
        for i in range(self.nb_mixtures):
            idx = np.flatnonzero(comp == i)
            if idx.size:
                out[idx] = r.multivariate_normal(self.mus[i], self.sigmas[i], size=idx.size)
        return out

    def log_density(self, X):
        from scipy.stats import multivariate_normal
        dens = [pi * multivariate_normal(mean=m, cov=sg).pdf(X)
                for pi, m, sg in zip(self.pis, self.mus, self.sigmas)]
        return np.log(np.sum(dens, axis=0))


class GaussianFunnel(object):
    """Neal's funnel, x_0 = v ~ N(0, sigma^2), x_k ~ N(0, e^v), with the energy clipped at
    |v| > 4 sigma  (distributions.py:155-198; sigma = 2)."""

    def __init__(self, dim=2, clip=6.):
        self.dim = dim
        self.sigma = 2.0
        self.clip = 4 * self.sigma

    def get_energy_function(self):
        return EnergyFunction(_ffi.ENERGY_FUNNEL, self.dim, eta=self.sigma)

    def get_samples(self, n, rng=None):
        r = _rng(rng)
        v = self.sigma * r.randn(n)
        rest = np.exp(v / 2)[:, None] * r.randn(n, self.dim - 1)
        return np.concatenate([v[:, None], rest], axis=1)

    def log_density(self, x):
        """Same expression as the reference's `log_density` (:190-198), in numpy throughout
        (the reference mixes tf ops into it)."""
        v = x[:, 0]
        n = x.shape[1] - 1
        ss = np.sum(x[:, 1:] ** 2, axis=1)
        return 0.5 * ((v / self.sigma) ** 2 + ss * np.exp(-v) + (n / 2) * (np.log(2 * np.pi) + v))


def gen_ring(r=1.0, var=1.0, nb_mixtures=2):
    """`nb_mixtures` isotropic components equally spaced on a circle of radius r (distributions.py:201-213)."""
    ang = 2 * np.pi * np.arange(nb_mixtures) / nb_mixtures
    centres = [np.array([r * np.cos(a), r * np.sin(a)]) for a in ang]
    covs = [var * np.eye(2) for _ in range(nb_mixtures)]
    w = [1. / nb_mixtures] * nb_mixtures
    w[0] += 1 - sum(w)                       # make the weights sum to exactly 1.0
    return GMM(centres, covs, w)
