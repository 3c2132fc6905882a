"""CPU stand-in for ``bayesml_amd._expfam.ExpfamPass`` (TEST INFRASTRUCTURE ONLY).

Implements the semantics of include/expfam.h in float64 / int64 torch on the CPU so that the HOST logic of the five scalar
conjugate models (type checks, refusal on ``bad``, closed forms, bookkeeping, pickle) can be tested without a GPU.  It is
injected through the private ``LearnModel._expfam_pass_factory`` seam by tests only; the product path never constructs it
and fails loudly without the HIP engine.
"""
import torch

from bayesml_amd import _expfam as xf


def _slots(ints=(), floats=()):
    return torch.cat([torch.tensor(list(ints), dtype=torch.int64),
                      torch.tensor(list(floats), dtype=torch.float64).view(torch.int64)])


class CpuExpfamPass:
    def __init__(self):
        self.device = torch.device("cpu")
        self.launch_info = "cpu stand-in"
        self.calls = []

    def adopt(self, a, kind, cols=None):
        # the product's own dtype plumbing, so that the seam cannot hide what it does to the caller's values
        return xf.adopt_tensor(a, self.device, kind, cols)

    def stats(self, family, x, degree=0):
        """As the expfam_stats_* entry points: x in a dtype the kernels read (anything else is refused), n >= 1."""
        self.calls.append((family, xf.code(x.dtype), tuple(x.shape)))
        assert x.shape[0] >= 1
        n = x.shape[0]
        if family in (xf.EXPONENTIAL, xf.NORMAL):
            assert x.dtype.is_floating_point and x.dim() == 1
            v = x.to(torch.float64)
            if family == xf.NORMAL:
                mean = v.sum() / n
                return torch.cat([_slots([n]), _slots(floats=[mean, ((v - mean) ** 2).sum()])])
            ok = v > 0
            return torch.cat([_slots([n, int((~ok).sum())]), _slots(floats=[v[ok].sum()])])
        assert not x.dtype.is_floating_point and x.dtype != torch.bool
        v = x.to(torch.int64)
        if family == xf.BERNOULLI:
            n1, n0 = int((v == 1).sum()), int((v == 0).sum())
            return _slots([n, n - n1 - n0, n1, n0])
        if family == xf.COUNTS:
            assert 1 <= degree <= xf.MAX_DEGREE
            ok = (v >= 0) & (v < degree)
            counts = torch.bincount(v[ok], minlength=degree)
            return torch.cat([_slots([n, int((~ok).sum()), int(v.max())]), counts])
        if family == xf.ONEHOT:
            assert 1 <= degree <= xf.MAX_DEGREE and x.dim() == 2 and x.shape[1] == degree
            ok = (v >= 0).all(dim=1) & (v.sum(dim=1) == 1)
            return torch.cat([_slots([n, int((~ok).sum())]), v[ok].sum(dim=0)])
        assert family == xf.POISSON and x.dim() == 1
        ok = v >= 0
        g = v[ok]
        return torch.cat([_slots([n, int((~ok).sum()), int(g.sum())]),
                          _slots(floats=[torch.lgamma(g.to(torch.float64) + 1.0).sum()])])

    def close(self):
        pass


def cpu_factory():
    return CpuExpfamPass()


def use_cpu(model):
    """``prepare`` of the oracle's driver: route a LearnModel's array updates through the stand-in."""
    model._expfam_pass_factory = cpu_factory
    return model
