"""A numpy CMA-ES with active (negative) recombination weights: the meta-optimizer of LES_Agent.

The reference uses ``cmaes.CMA(mean, sigma, population_size)``; that package is not a dependency here, so this module restates its equations
(N. Hansen, "The CMA Evolution Strategy: A Tutorial", 2016, in the form the package uses: eq. numbers below are the tutorial's).  What is pinned
against the reference: every derived constant equals the one recorded in the reference's shipped LES checkpoints (tests/test_les.py).  The
trajectory is NOT pinned: the package's own random stream is not reproduced.
"""
import math

import numpy as np

_EPS = 1e-8
_SIGMA_MAX = 1e32


class CMA:
    def __init__(self, mean, sigma, population_size=None, seed=None):
        mean = np.array(mean, dtype=np.float64)
        n = len(mean)
        assert n > 1 and sigma > 0
        if population_size is None:
            population_size = 4 + math.floor(3 * math.log(n))
        assert population_size > 0
        lam = int(population_size)
        mu = lam // 2
        wp = np.array([math.log((lam + 1) / 2) - math.log(i + 1) for i in range(lam)])
        mu_eff = (np.sum(wp[:mu]) ** 2) / np.sum(wp[:mu] ** 2)
        mu_eff_minus = (np.sum(wp[mu:]) ** 2) / np.sum(wp[mu:] ** 2)
        alpha_cov = 2
        c1 = alpha_cov / ((n + 1.3) ** 2 + mu_eff)
        cmu = min(1 - c1 - 1e-8, alpha_cov * (mu_eff - 2 + 1 / mu_eff) / ((n + 2) ** 2 + alpha_cov * mu_eff / 2))
        assert c1 <= 1 - cmu and cmu <= 1 - c1
        min_alpha = min(1 + c1 / cmu,                               # eq. 50
                        1 + (2 * mu_eff_minus) / (mu_eff + 2),      # eq. 51
                        (1 - c1 - cmu) / (n * cmu))                 # eq. 52
        positive_sum = np.sum(wp[wp > 0])
        negative_sum = np.sum(np.abs(wp[wp < 0]))
        self._weights = np.where(wp >= 0, 1 / positive_sum * wp, min_alpha / negative_sum * wp)
        self._n_dim, self._popsize, self._mu, self._mu_eff = n, lam, mu, mu_eff
        self._c1, self._cmu, self._cm = c1, cmu, 1
        self._c_sigma = (mu_eff + 2) / (n + mu_eff + 5)                                            # eq. 55
        self._d_sigma = 1 + 2 * max(0, math.sqrt((mu_eff - 1) / (n + 1)) - 1) + self._c_sigma
        assert self._c_sigma < 1
        self._cc = (4 + mu_eff / n) / (n + 4 + 2 * mu_eff / n)                                     # eq. 56
        assert self._cc <= 1
        self._chi_n = math.sqrt(n) * (1.0 - (1.0 / (4.0 * n)) + 1.0 / (21.0 * (n ** 2)))           # E||N(0, I)||
        self._p_sigma, self._pc = np.zeros(n), np.zeros(n)
        self._mean, self._sigma, self._C = mean, float(sigma), np.eye(n)
        self._B = self._D = None
        self._g = 0
        self._rng = np.random.RandomState(seed)

    @property
    def dim(self):
        return self._n_dim

    @property
    def population_size(self):
        return self._popsize

    @property
    def generation(self):
        return self._g

    @property
    def mean(self):
        return self._mean.copy()

    @property
    def sigma(self):
        return self._sigma

    def _eigen_decomposition(self):
        if self._B is not None and self._D is not None:
            return self._B, self._D
        self._C = (self._C + self._C.T) / 2
        D2, B = np.linalg.eigh(self._C)
        D = np.sqrt(np.where(D2 < 0, _EPS, D2))
        self._C = np.dot(np.dot(B, np.diag(D ** 2)), B.T)
        self._B, self._D = B, D
        return B, D

    def ask(self):
        """One sample of N(mean, sigma^2 C); the eigen-decomposition is refreshed here after a tell."""
        B, D = self._eigen_decomposition()
        z = self._rng.randn(self._n_dim)
        y = B.dot(np.diag(D)).dot(z)
        return self._mean + self._sigma * y

    def tell(self, solutions):
        """solutions: population_size pairs (x, value); lower values are better."""
        assert len(solutions) == self._popsize, 'Must tell popsize-length solutions.'
        for s in solutions:
            assert np.all(np.abs(s[0]) < 1e32), 'Absolute value of all generated solutions must be less than 1e32'
        self._g += 1
        solutions = sorted(solutions, key=lambda s: s[1])
        B, D = self._eigen_decomposition()
        self._B = self._D = None
        x_k = np.array([s[0] for s in solutions])
        y_k = (x_k - self._mean) / self._sigma
        y_w = np.sum(y_k[:self._mu].T * self._weights[:self._mu], axis=1)                          # eq. 41
        self._mean = self._mean + self._cm * self._sigma * y_w
        C_2 = B.dot(np.diag(1 / D)).dot(B.T)                                                       # C^(-1/2)
        self._p_sigma = (1 - self._c_sigma) * self._p_sigma + math.sqrt(self._c_sigma * (2 - self._c_sigma) * self._mu_eff) * C_2.dot(y_w)
        norm_p_sigma = np.linalg.norm(self._p_sigma)
        self._sigma *= np.exp((self._c_sigma / self._d_sigma) * (norm_p_sigma / self._chi_n - 1))
        self._sigma = min(self._sigma, _SIGMA_MAX)
        h_left = norm_p_sigma / math.sqrt(1 - (1 - self._c_sigma) ** (2 * (self._g + 1)))
        h_right = (1.4 + 2 / (self._n_dim + 1)) * self._chi_n
        h_sigma = 1.0 if h_left < h_right else 0.0
        self._pc = (1 - self._cc) * self._pc + h_sigma * math.sqrt(self._cc * (2 - self._cc) * self._mu_eff) * y_w     # eq. 45
        w_io = self._weights * np.where(self._weights >= 0, 1, self._n_dim / (np.linalg.norm(C_2.dot(y_k.T), axis=0) ** 2 + _EPS))   # eq. 46
        delta_h_sigma = (1 - h_sigma) * self._cc * (2 - self._cc)
        assert delta_h_sigma <= 1
        rank_one = np.outer(self._pc, self._pc)
        rank_mu = (y_k.T * w_io).dot(y_k)                                                          # sum_i w_i y_i y_i^T
        self._C = ((1 + self._c1 * delta_h_sigma - self._c1 - self._cmu * np.sum(self._weights)) * self._C
                   + self._c1 * rank_one + self._cmu * rank_mu)                                    # eq. 47
