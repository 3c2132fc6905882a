"""CPU stand-in for ``bayesml_amd._regression.RegressionPass`` (TEST INFRASTRUCTURE ONLY).

Implements the semantics of include/regvb.h in float64 torch on the CPU so that the HOST logic of linearregression /
autoregressive (validation, closed-form update, lazy predictive arrays, pickle) can be tested without a GPU.  It is
injected through the private ``LearnModel._reg_pass_factory`` seam by tests only; the product path never constructs
it and fails loudly without the HIP engine.
"""
import numpy as np
import torch


class CpuRegressionPass:
    def __init__(self, D):
        self.D = D
        self.device = torch.device("cpu")
        self.stats_len = D * D + D + 2
        self.launch_info = "cpu stand-in"

    def adopt(self, a):
        # the product's own dtype plumbing, so that the seam cannot hide what it does to the caller's values
        from bayesml_amd._regression import adopt_tensor
        return adopt_tensor(a, self.device)

    @staticmethod
    def _block(w, y):
        w, y = w.to(torch.float64), y.to(torch.float64)
        n = torch.tensor([float(w.shape[0])], dtype=torch.float64)
        return torch.cat([(w.T @ w).reshape(-1), w.T @ y, (y @ y).reshape(1), n])

    def stats(self, x, y):
        """As regvb_stats: x and y in their own dtypes (f32 or f64, anything else is refused), each widened, none narrowed."""
        from bayesml_amd._regression import _code
        assert x.dim() == 2 and x.shape[1] == self.D and y.shape == (x.shape[0],)
        self.last_dtypes = (_code(x.dtype), _code(y.dtype))
        return self._block(x, y)

    def stats_window(self, series, padding):
        p = self.D - 1
        s = series.to(torch.float64)
        T = s.shape[0]
        assert s.dim() == 1 and T > p and padding in (0, 1)
        sp = torch.cat([torch.zeros(p, dtype=torch.float64), s])
        w = torch.ones((T, p + 1), dtype=torch.float64)
        for k in range(p):
            w[:, 1 + k] = sp[k:k + T]
        t0 = 0 if padding == 1 else p
        return self._block(w[t0:], s[t0:])

    def predict(self, x, mu, linv, scale):
        assert x.dim() == 2 and x.shape[1] == self.D
        x = x.to(torch.float64)
        z = x @ torch.from_numpy(np.tril(linv)).T
        return x @ torch.from_numpy(np.asarray(mu, dtype=np.float64)), scale / (1.0 + (z * z).sum(dim=1))

    def close(self):
        pass


def cpu_factory(D):
    return CpuRegressionPass(D)
