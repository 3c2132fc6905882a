"""gmmvb_mstep as it is planned (bayesml_amd/csrc/mstep_plan.h) on the device: its refusals, the GMMVB_MLIST_XC switch and the
launch geometry of every form.  tests/test_mstep_plan.py holds every branch of the plan to the old code without a GPU.

Refusals.  Four of the five GMMVB_ESTATE answers of gmmvb_mstep can be reached through DataPass's methods; each is held to its
code and text, and the workspace must carry on as if the refused call had not been made: its next estep_mstep gives, bit for
bit, what a twin workspace gives that went through the same calls without the refused one (and, to 1e-12 relative, the
statistics it gave before: the same sums under the same parameters, through another pass).  The fifth - "settled rows need the
list M-step ..." (lock_live without lists) - cannot be reached that way: rows only settle in a pruned E-step, whose output
(rec_live) is refused first with its own message, and everything that ends rec_live (a dense E-step, loaded
responsibilities, new rows or pivot, another tile's turn) drops the settled rows or the responsibilities with it.  It is left
to the host cases.

Geometry.  The M-step's segment of launch_info is a literal, recorded on the commit before the plan was moved out of
gmmvb_mstep: with unchanged kernels and no atomics, equal geometry means equal bits."""
import warnings

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import gmm_vb_oracle as orc

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
NO_RESP = "no responsibilities for these rows: call gmmvb_estep or gmmvb_load_responsibilities first"
REGROUPED = "the workspace's rows are regrouped for another sample matrix: call gmmvb_prepare_rows first"
PRUNED = "a pruned E-step needs the list M-step over the matrix of the E-step (gmmvb_prepare_rows)"
LOST = "the M-step's lists were used by a read-out of settled rows: call gmmvb_estep again"


def dev():
    return torch.device("cuda", 0)


def features(K, D, x):
    """Device parameters of the oracle's subsampling initialisation (as __graft_entry__.smoke)."""
    from bayesml_amd import _kside
    q = orc.Posterior.from_prior(orc.Prior.default(K, D))
    orc.init_subsampling(x.astype(np.float64), q, np.random.default_rng(0))
    t = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev())   # noqa: E731
    return _kside.features(_kside.PostT(t(q.alpha), t(q.m), t(q.kappa), t(q.nu), t(q.w_inv)))


def workspace(K, D, x, prepare=True, max_rows=None, params=None):
    from bayesml_amd._engine import DataPass
    xd = torch.from_numpy(np.array(x)).to(dev())
    eng = DataPass(K, D, xd.dtype, max_rows or x.shape[0], dev())
    eng.set_pivot(xd[:4096].to(torch.float64).mean(dim=0))
    if prepare:
        eng.prepare_rows(xd)
    if params is not None:
        eng.set_params(params.c, params.m, params.u)
    return eng, xd


def forced_fit(K, D, N, max_itr):
    from bayesml_amd import gaussianmixture as gm
    x = orc.synth_gmm(K, D, N, F32)
    m = gm.LearnModel(K, D, seed=0, device=dev(), verbose=False)
    eng, xd = m._open(x)
    eng.lib.gmmvb_policy_calibrate(eng._ws, 0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.update_posterior(xd, max_itr=max_itr, num_init=1, tolerance=0.0)
    assert m._engine is eng
    return m, eng, xd


def refused(eng, x, message):
    from bayesml_amd._engine import EngineError
    with pytest.raises(EngineError) as err:
        eng.mstep(x)
    assert str(err.value) == f"gmmvb_mstep: GMMVB_ESTATE: {message}"


def next_pass(eng, xd):
    """The workspace's next estep_mstep, once the device is idle: the E-step chooses its kind of pass from the counters of the
    previous one that have ARRIVED, and a refused call in between must not be what gives them the time to."""
    torch.cuda.synchronize()
    return eng.estep_mstep(xd).clone()


def same_after(tag, after, twin, before=None):
    if before is not None:
        print("mstep-plan", tag, "rel to the statistics before:", rel_err(after.cpu().numpy(), before.cpu().numpy()))
        assert rel_err(after.cpu().numpy(), before.cpu().numpy()) < 1e-12
    assert torch.equal(after, twin)


# ---- a. refusals ---------------------------------------------------------------------------------------------------------
def test_refused_without_responsibilities():
    K, D, N = 6, 64, 6000
    x = orc.synth_gmm(K, D, N, F32)
    qd = features(K, D, x)
    out = []
    for refuse in (True, False):
        eng, xd = workspace(K, D, x, params=qd)
        if refuse:
            refused(eng, xd, NO_RESP)
        out.append(next_pass(eng, xd))
        eng.close()
    same_after("fresh", *out)


def test_refused_after_a_pruned_estep_over_another_matrix(monkeypatch):
    """A pruned E-step's output (exact ln rho for the listed pairs only) needs the list M-step, which needs the prepared rows:
    a copy of the matrix at another address is another matrix."""
    monkeypatch.setenv("GMMVB_ESTEP_PRUNE", "force")
    K, D, N = 6, 64, 6000
    x = orc.synth_gmm(K, D, N, F32)
    qd = features(K, D, x)
    out = []
    for refuse in (True, False):
        eng, xd = workspace(K, D, x, params=qd)
        eng.estep(xd)
        assert "estep_i8_bound" in eng.launch_info
        if refuse:
            refused(eng, xd.clone(), PRUNED)
        before = eng.mstep(xd).clone()                 # (the matrix of the E-step is still served)
        out.append(next_pass(eng, xd))
        eng.close()
    same_after("pruned", *out, before=before)


def test_refused_over_rows_regrouped_for_another_matrix(monkeypatch):
    monkeypatch.setenv("GMMVB_ESTEP_PRUNE", "force")
    K, D, N = 70, 64, 6000
    out = []
    for refuse in (True, False):
        _m, eng, xd = forced_fit(K, D, N, 4)
        assert eng.regroup_count == 1
        before = eng.estep_mstep(xd).clone()
        eng.load_responsibilities(eng.responsibilities(0, N).clone())
        if refuse:
            refused(eng, xd.clone(), REGROUPED)
        out.append(next_pass(eng, xd))
    same_after("regrouped", *out, before=before)


def test_refused_after_a_readout_of_settled_rows(monkeypatch):
    """The read-out of settled rows builds its lists where the M-step's were: a second M-step of the same E-step is refused."""
    monkeypatch.setenv("GMMVB_ESTEP_PRUNE", "force")
    K, D, N = 6, 64, 6000
    out = []
    for refuse in (True, False):
        _m, eng, xd = forced_fit(K, D, N, 4)
        before = eng.estep_mstep(xd).clone()
        eng.responsibilities(0, N)
        if refuse:
            refused(eng, xd, LOST)
        out.append(next_pass(eng, xd))
    same_after("lists lost", *out, before=before)


# ---- b. the developer switch ---------------------------------------------------------------------------------------------
def test_mlist_xc_switch(monkeypatch):
    """GMMVB_MLIST_XC=1 (behind GMMVB_DEBUG, read when the workspace is created): the list kernel over the centred f64 copy
    instead of the f32 rows - two kernels doing the same sums."""
    monkeypatch.setenv("GMMVB_ESTEP_PRUNE", "force")
    K, D, N = 8, 64, 6000
    x = orc.synth_gmm(K, D, N, F32)
    qd = features(K, D, x)
    stats = {}
    for on, want in ((True, "mstep_list_f64<T=4,centred-f64>"), (False, "mstep_list_f64<T=4,x=f32>")):
        if on:
            monkeypatch.setenv("GMMVB_DEBUG", "1")
            monkeypatch.setenv("GMMVB_MLIST_XC", "1")
        else:
            monkeypatch.delenv("GMMVB_DEBUG", raising=False)
            monkeypatch.delenv("GMMVB_MLIST_XC", raising=False)
        eng, xd = workspace(K, D, x, params=qd)
        stats[on] = eng.estep_mstep(xd).cpu().numpy()
        assert want in eng.launch_info, eng.launch_info
        eng.close()
    print("mstep-plan MLIST_XC rel", rel_err(stats[True], stats[False]))
    assert rel_err(stats[True], stats[False]) < 1e-12


# ---- c. pinned launch geometry -------------------------------------------------------------------------------------------
def segment(eng):
    return eng.launch_info.split(" | ")[-1]


def loaded(K, D, N, dtype, max_rows=None):
    x = orc.synth_gmm(K, D, N, dtype)
    eng, xd = workspace(K, D, x, prepare=False, max_rows=max_rows)
    eng.load_responsibilities(torch.from_numpy(np.random.default_rng(K + D).dirichlet(0.3 * np.ones(K), N)).to(dev()))
    eng.mstep(xd)
    seg = segment(eng)
    eng.close()
    return seg


def after_estep(K, D, N, dtype):
    x = orc.synth_gmm(K, D, N, dtype)
    eng, xd = workspace(K, D, x, params=features(K, D, x))
    eng.estep_mstep(xd)
    seg = segment(eng)
    eng.close()
    return seg


def test_dense_geometry():
    assert after_estep(5, 40, 257, F64) == "mstep_mfma_f64<T=3,centred-f64> grid=16x256 splits=5 rows/split=64"
    assert loaded(3, 40, 65, F64) == "mstep_mfma_f64<T=3,x=f64,masked> grid=8x256 splits=2 rows/split=64"
    assert loaded(5, 64, 257, F32) == "mstep_mfma_f64<T=4,x=f32,vec> grid=16x256 splits=5 rows/split=64"
    assert after_estep(5, 16, 300, F32) == "mstep_small_f64<T=1,8 components per wave,centred-f64> grid=8x256 splits=5 rows/split=64"
    # no gmmvb_prepare_rows: the M-step makes the centred copy itself
    assert loaded(4, 129, 600, F32) == "mstep_wide_f64<T=10,centred-f64,5 waves per component> grid=64x320 splits=10 rows/split=64"
    assert loaded(3, 257, 300, F64) == "mstep_generic_f64<D=257> tiles=153 splits=1"
    assert loaded(3, 257, 300, F64, max_rows=40000) == "mstep_generic_f64<D=257> tiles=153 splits=2"


def test_list_geometry_before_and_after_the_regrouping(monkeypatch):
    """The K = 8 forced fit regroups its rows in its second pass: the lists read the caller's f32 rows before, the
    workspace's regrouped copy after - the same kernel, grid and chunk length."""
    monkeypatch.setenv("GMMVB_ESTEP_PRUNE", "force")
    from bayesml_amd._engine import DataPass
    seen = []
    inner = DataPass.estep_mstep

    def noted(self, *a, **k):
        out = inner(self, *a, **k)
        seen.append((self.regroup_count, segment(self)))
        return out

    monkeypatch.setattr(DataPass, "estep_mstep", noted)
    forced_fit(8, 64, 6000, 3)
    want = "mstep_list_f64<T=4,x=f32> grid=14x256 splits=0 rows/split=1024"
    assert seen == [(0, want), (1, want), (1, want), (1, want)]


def test_list_geometry_over_f64_rows(monkeypatch):
    """f64 rows at three feature tiles have no pruned E-step: the lists follow a counted dense E-step (N K >= 2^18) that left
    few pairs active - clusters 8 standard deviations apart per feature, parameters at their means."""
    monkeypatch.setenv("GMMVB_ESTEP_PRUNE", "force")
    from bayesml_amd import _kside
    K, D, N = 6, 40, 44032
    x = orc.synth_gmm(K, D, N, F64, spread=8.0)
    mu = 8.0 * np.random.default_rng(20250711).standard_normal((K, D))        # synth_gmm's own means
    t = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev())   # noqa: E731
    qd = _kside.features(_kside.PostT(t(np.full(K, N / K)), t(mu), t(np.full(K, 100.0)), t(np.full(K, D + 100.0)),
                                      t(np.tile((D + 100.0) * np.eye(D), (K, 1, 1)))))
    eng, xd = workspace(K, D, x, params=qd)
    eng.estep_mstep(xd)
    active, _evaluated = eng.sparsity()
    seg, counts = segment(eng), eng.pass_counts()
    eng.close()
    print("mstep-plan f64 lists: active pairs", active, "of", N * K)
    assert active < 0.5 * N * K and counts["mstep_list"] == 1
    assert seg == "mstep_list_f64<T=3,centred-f64> grid=66x256 splits=0 rows/split=1024"
