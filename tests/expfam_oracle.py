"""What the fixtures of the five scalar conjugate models and their tests share (TEST INFRASTRUCTURE ONLY):

* the seeded recipes of the samples that are not stored (tests/golden/make_golden_expfam.py stores a recipe's arguments
  and a checksum of what it made; ``batches`` re-makes and verifies it),
* ``CASES``, the fixture definitions,
* ``drive``, the one walk over a model package's public API whose results the generator records from the reference and
  the tests compare against the drop-in, key by key,
* ``error_cases``, the boundary inputs whose outcome (exception class name or None) is recorded in expfam_errors.json.
"""
import json
import warnings
import zlib

import numpy as np

EPS = float(np.finfo(np.float64).eps)
LOSSES = {"bernoulli": ("squared", "0-1", "abs", "KL"), "categorical": ("squared", "0-1", "KL"),
          "poisson": ("squared", "0-1", "abs", "KL"), "exponential": ("squared", "0-1", "abs", "KL"),
          "normal": ("squared", "0-1", "abs", "KL")}
N_SEQ = 20


# ---- samples ---------------------------------------------------------------------------------------------------------
def checksum(a):
    """What a fixture stores of a recipe-made array: the CRC of its bytes."""
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def make(recipe):
    """A sample from its recipe.  Only the Generator's own stream and element-wise arithmetic are used (no reductions),
    so every machine makes the same bits; the stored checksum says so."""
    r = dict(recipe)
    kind, n, dtype = r["kind"], int(r["n"]), np.dtype(r["dtype"])
    rng = np.random.default_rng(int(r["seed"]))
    if kind == "bernoulli":
        return (rng.random(n) < r["p"]).astype(dtype)
    if kind == "index":
        return rng.integers(0, int(r["degree"]), n).astype(dtype)
    if kind == "onehot":
        idx = rng.integers(0, int(r["degree"]), n)
        x = np.zeros((n, int(r["degree"])), dtype=dtype)
        x[np.arange(n), idx] = 1
        return x
    if kind == "poisson":
        x = rng.poisson(r["lam"], n).astype(np.int64)
        for i, v in enumerate(r.get("plant", [])):          # special values at fixed, spread positions
            x[(i * 7919 + 3) % n] = v
        if dtype == np.uint8:
            x = np.minimum(x, 255)
        return x.astype(dtype)
    if kind == "exponential":
        x = rng.exponential(r["scale"], n).astype(dtype)
        return np.maximum(x, np.finfo(dtype).tiny)
    if kind == "normal":
        return (r["loc"] + r["scale"] * rng.standard_normal(n)).astype(dtype)
    raise ValueError(kind)


def widen(a):
    """What the reference is fed: the int64 / float64 widening of the same values."""
    return a.astype(np.int64 if a.dtype.kind in "iu" else np.float64)


def _poisson_plant():
    return [0, 1, 2, 170, 171, 10 ** 6, 10 ** 9, 2 ** 40]


# name -> (family, constructor args, prior kwargs, update kwargs, recipes of the two batches or None = drawn from GenModel)
CASES = {
    "expfam_bernoulli_gen_n50": ("bernoulli", (), {}, {}, None),
    "expfam_bernoulli_u8_n100003": ("bernoulli", (), dict(h0_alpha=2.5, h0_beta=0.75), {}, [
        dict(kind="bernoulli", n=100003, seed=101, p=0.3, dtype="uint8"),
        dict(kind="bernoulli", n=4097, seed=102, p=0.6, dtype="uint8")]),
    "expfam_bernoulli_i32_n70001": ("bernoulli", (), {}, {}, [
        dict(kind="bernoulli", n=70001, seed=103, p=0.01, dtype="int32"),
        dict(kind="bernoulli", n=257, seed=104, p=0.5, dtype="int32")]),
    "expfam_categorical_gen_d3_n40": ("categorical", (3,), {}, {}, None),
    "expfam_categorical_onehot_d16_u8_n20000": ("categorical", (16,), dict(h0_alpha_vec=2.0), {}, [
        dict(kind="onehot", n=20000, seed=111, degree=16, dtype="uint8"),
        dict(kind="onehot", n=1025, seed=112, degree=16, dtype="uint8")]),
    "expfam_categorical_index_d5_i32_n100003": ("categorical", (5,), {}, dict(onehot=False), [
        dict(kind="index", n=100003, seed=113, degree=5, dtype="int32"),
        dict(kind="index", n=4097, seed=114, degree=5, dtype="int32")]),
    "expfam_categorical_index_d1000_n50000": ("categorical", (1000,), dict(h0_alpha_vec=0.1), dict(onehot=False), [
        dict(kind="index", n=50000, seed=115, degree=1000, dtype="int64"),
        dict(kind="index", n=4097, seed=116, degree=1000, dtype="int64")]),
    "expfam_poisson_gen_n60": ("poisson", (), {}, {}, None),
    "expfam_poisson_planted_n100003": ("poisson", (), dict(h0_alpha=2.0, h0_beta=0.5), {}, [
        dict(kind="poisson", n=100003, seed=121, lam=3.0, dtype="int64", plant=_poisson_plant()),
        dict(kind="poisson", n=4097, seed=122, lam=50.0, dtype="int64")]),
    "expfam_poisson_u8_n70001": ("poisson", (), {}, {}, [
        dict(kind="poisson", n=70001, seed=123, lam=20.0, dtype="uint8"),
        dict(kind="poisson", n=257, seed=124, lam=200.0, dtype="int32")]),
    "expfam_exponential_gen_n50": ("exponential", (), {}, {}, None),
    "expfam_exponential_f32_n100003": ("exponential", (), dict(h0_alpha=3.0, h0_beta=2.0), {}, [
        dict(kind="exponential", n=100003, seed=131, scale=2.0, dtype="float32"),
        dict(kind="exponential", n=4097, seed=132, scale=0.5, dtype="float32")]),
    "expfam_exponential_f64_n70001": ("exponential", (), {}, {}, [
        dict(kind="exponential", n=70001, seed=133, scale=1e-3, dtype="float64"),
        dict(kind="exponential", n=257, seed=134, scale=1e-3, dtype="float64")]),
    "expfam_normal_gen_n50": ("normal", (), {}, {}, None),
    "expfam_normal_f64_1e8_n100003": ("normal", (), {}, {}, [
        dict(kind="normal", n=100003, seed=141, loc=1e8, scale=1.0, dtype="float64"),
        dict(kind="normal", n=4097, seed=142, loc=1e8, scale=1.0, dtype="float64")]),
    "expfam_normal_f64_1e4_n70001": ("normal", (), dict(h0_m=1e4, h0_kappa=2.0, h0_alpha=1.5, h0_beta=0.5), {}, [
        dict(kind="normal", n=70001, seed=143, loc=1e4, scale=0.01, dtype="float64"),
        dict(kind="normal", n=4097, seed=144, loc=1e4, scale=0.01, dtype="float64")]),
    "expfam_normal_f32_n100003": ("normal", (), {}, {}, [
        dict(kind="normal", n=100003, seed=145, loc=3.0, scale=2.0, dtype="float32"),
        dict(kind="normal", n=4097, seed=146, loc=3.0, scale=2.0, dtype="float32")]),
    "expfam_normal_f64_m5e5_n4097": ("normal", (), {}, {}, [
        dict(kind="normal", n=4097, seed=147, loc=-5e5, scale=0.5, dtype="float64"),
        dict(kind="normal", n=65, seed=148, loc=-5e5, scale=0.5, dtype="float64")]),
}
GEN_SEED = 7
GEN_SIZES = {"expfam_bernoulli_gen_n50": (50, 30), "expfam_categorical_gen_d3_n40": (40, 25),
             "expfam_poisson_gen_n60": (60, 30), "expfam_exponential_gen_n50": (50, 30), "expfam_normal_gen_n50": (50, 30)}
GEN_KW = {"bernoulli": dict(theta=0.3), "categorical": dict(theta_vec=np.array([0.2, 0.5, 0.3])), "poisson": dict(lambda_=4.0),
          "exponential": dict(lambda_=2.0), "normal": dict(mu=-1.5, tau=4.0)}


def gen_batches(mod, name):
    """The two batches of a *_gen_* case: the model package's own GenModel, seeded (the drop-in's must draw the same)."""
    family, ctor = CASES[name][0], CASES[name][1]
    g = mod.GenModel(*ctor, seed=GEN_SEED, **GEN_KW[family])
    return [g.gen_sample(n) for n in GEN_SIZES[name]]


def batches(name, fixture):
    """The two batches of a case: stored ones, or re-made from the recipe and verified against the stored checksums."""
    recipes = CASES[name][4]
    if recipes is None:
        return [fixture["x0"], fixture["x1"]]
    out = [make(r) for r in recipes]
    for i, b in enumerate(out):
        assert checksum(b) == int(fixture[f"checksum{i}"]), "the sample recipe no longer reproduces the fixture's sample"
    return out


# ---- the walk over a model's API -------------------------------------------------------------------------------------
def _flat(out, key, v, as_array):
    """Record a returned value under ``key``: None -> nan, a frozen scipy distribution -> its mean and variance, a tuple
    -> its elements."""
    if isinstance(v, tuple):
        for i, e in enumerate(v):
            _flat(out, f"{key}_{i}", e, as_array)
    elif v is None:
        out[key] = as_array(np.nan)
    elif hasattr(v, "mean") and hasattr(v, "var") and not isinstance(v, (np.ndarray, np.generic)):
        out[key + "_mean"] = as_array(v.mean())
        out[key + "_var"] = as_array(v.var())
    else:
        out[key] = as_array(v)


def seq_items(family, update_kw, b0):
    """The N_SEQ single observations of the pred_and_update sequence: Python scalars, or one-hot rows."""
    if family == "categorical" and update_kw.get("onehot", True):
        return [np.asarray(r).astype(np.int64) for r in b0[:N_SEQ]]
    return [v.item() for v in np.asarray(b0).reshape(-1)[:N_SEQ]]


def drive(mod, name, bs, prepare=None, to_input=None, as_array=None, lenient=False):
    """Everything the fixtures hold of one case, from the model package ``mod``: a dict key -> array.  ``bs`` are the two
    batches, ``to_input`` turns a batch into what update_posterior is given, ``prepare`` is applied to every LearnModel.
    With ``lenient`` a quantity the model cannot evaluate (TypeError) is left out."""
    family, ctor, prior, ukw, _ = CASES[name]
    to_input = to_input or (lambda a: a)
    as_array = as_array or (lambda v: np.asarray(v, dtype=np.float64))
    out = {}

    def attempt(fn):
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                fn()
        except TypeError:
            if not lenient:
                raise

    def new():
        m = mod.LearnModel(*ctor, **prior)
        if prepare is not None:
            prepare(m)
        return m

    m = new()
    for i, b in enumerate(bs):
        m.update_posterior(to_input(b), **ukw)
        for k, v in m.get_hn_params().items():
            out[f"b{i}_{k}"] = as_array(v).copy()
    for loss in LOSSES[family]:
        attempt(lambda: _flat(out, f"est_{loss}", m.estimate_params(loss), as_array))
    out["est_keys"] = json.dumps(list(m.estimate_params("squared", dict_out=True)))
    if hasattr(m, "estimate_interval"):
        attempt(lambda: _flat(out, "interval", m.estimate_interval(0.9), as_array))
    m.calc_pred_dist()
    for k, v in m.get_p_params().items():
        out["pp_" + k] = as_array(v).copy()
    for loss in LOSSES[family]:
        attempt(lambda: _flat(out, f"pred_{loss}", m.make_prediction(loss), as_array))
    if family == "categorical":
        out["pred_0-1_index"] = as_array(m.make_prediction("0-1", onehot=False))
    attempt(lambda: _flat(out, "lml", m.calc_log_marginal_likelihood(), as_array))
    if hasattr(m, "calc_pred_var"):
        attempt(lambda: _flat(out, "pred_var", m.calc_pred_var(), as_array))
    if hasattr(m, "predict_proba"):
        out["predict_proba"] = as_array(m.predict_proba()).copy()
    attempt(lambda: _flat(out, "predict", m.predict(), as_array))
    out["key_order"] = json.dumps([list(m.get_constants()), list(m.get_h0_params()), list(m.get_hn_params()),
                                   list(m.get_p_params())])
    # the sequence: N_SEQ single observations, predicted (squared loss) and folded in one by one, host work only
    s = new()
    preds = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for item in seq_items(family, ukw, bs[0]):
            p = s.pred_and_update(item, **ukw)
            preds.append(as_array(np.nan if p is None else p).copy())
    out["seq_preds"] = np.stack(preds)
    for k, v in s.get_hn_params().items():
        out["seq_" + k] = as_array(v).copy()
    attempt(lambda: _flat(out, "seq_lml", s.calc_log_marginal_likelihood(), as_array))
    return out


def merge_normal(a, b):
    """The block of the union of two normal samples (include/expfam.h), on decoded dicts."""
    n = a["n"] + b["n"]
    d = b["mean"] - a["mean"]
    return dict(n=n, mean=a["mean"] + d * b["n"] / n, m2=a["m2"] + b["m2"] + d * d * a["n"] * b["n"] / n)


def is_number_key(k):
    return k not in ("est_keys", "key_order")


def rel_err(a, b):
    """max|a - b| / max|b| over the finite entries (nan and inf must sit in the same places)."""
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    fin = np.isfinite(b)
    if not np.array_equal(fin, np.isfinite(a)) or not np.array_equal(np.asarray(a)[~fin], np.asarray(b)[~fin], equal_nan=True):
        return float("inf")
    if not fin.any():
        return 0.0
    den = np.max(np.abs(b[fin]))
    return float(np.max(np.abs(a[fin] - b[fin])) / (den if den > 0 else 1.0))


def compare(name, got, fixture):
    """Every recorded quantity within the tolerance the fixture carries (max(8 x the reference's own error, 32 eps))."""
    keys = [k for k in fixture if not k.startswith(("err__", "tol__", "checksum", "x0", "x1"))]
    assert sorted(keys) == sorted(got), (name, set(keys) ^ set(got))
    for k in keys:
        if not is_number_key(k):
            assert str(fixture[k]) == got[k], (name, k)
            continue
        assert np.shape(got[k]) == fixture[k].shape, (name, k)
        err, tol = rel_err(got[k], fixture[k]), float(fixture["tol__" + k])
        assert err <= tol, (name, k, err, tol)


# ---- boundary cases --------------------------------------------------------------------------------------------------
def error_cases(mods, prepare=None):
    """name -> thunk.  ``mods`` maps a family name to its package; ``prepare`` is applied to every LearnModel made."""
    def lm(family, *a, **k):
        m = mods[family].LearnModel(*a, **k)
        if prepare is not None:
            prepare(m)
        return m
    i64 = np.int64
    return {
        "bernoulli_float_array": lambda: lm("bernoulli").update_posterior(np.array([0.0, 1.0])),
        "bernoulli_bool_array": lambda: lm("bernoulli").update_posterior(np.array([True, False])),
        "bernoulli_list": lambda: lm("bernoulli").update_posterior([0, 1]),
        "bernoulli_two": lambda: lm("bernoulli").update_posterior(np.array([0, 1, 2, 1], dtype=i64)),
        "bernoulli_negative": lambda: lm("bernoulli").update_posterior(np.array([0, -1, 1], dtype=i64)),
        "bernoulli_scalar_two": lambda: lm("bernoulli").update_posterior(2),
        "bernoulli_scalar_ok": lambda: lm("bernoulli").update_posterior(1),
        "bernoulli_2d_ok": lambda: lm("bernoulli").update_posterior(np.array([[0, 1], [1, 1]], dtype=i64)),
        "bernoulli_pred_float": lambda: lm("bernoulli").pred_and_update(1.0),
        "bernoulli_h0_alpha_zero": lambda: lm("bernoulli", h0_alpha=0.0),
        "bernoulli_h0_beta_negative": lambda: lm("bernoulli", h0_beta=-1.0),
        "bernoulli_h0_alpha_int_ok": lambda: lm("bernoulli", h0_alpha=2),
        "bernoulli_bad_loss_estimate": lambda: lm("bernoulli").estimate_params("L1"),
        "bernoulli_bad_loss_prediction": lambda: lm("bernoulli").make_prediction("L1"),
        "bernoulli_interval_out_of_range": lambda: lm("bernoulli").estimate_interval(1.5),
        "bernoulli_gen_theta_out_of_range": lambda: mods["bernoulli"].GenModel(theta=1.5),
        "bernoulli_gen_float_size": lambda: mods["bernoulli"].GenModel().gen_sample(3.0),
        "categorical_row_all_zero": lambda: lm("categorical", 3).update_posterior(np.array([[1, 0, 0], [0, 0, 0]], dtype=i64)),
        "categorical_row_two_ones": lambda: lm("categorical", 3).update_posterior(np.array([[1, 1, 0], [0, 0, 1]], dtype=i64)),
        "categorical_row_negative_sum_one": lambda: lm("categorical", 3).update_posterior(np.array([[0, 1, 0], [2, -1, 0]], dtype=i64)),
        "categorical_row_ok": lambda: lm("categorical", 3).update_posterior(np.array([0, 0, 1], dtype=i64)),
        "categorical_single_row_2d_ok": lambda: lm("categorical", 3).update_posterior(np.array([[0, 0, 1]], dtype=i64)),
        "categorical_3d_ok": lambda: lm("categorical", 2).update_posterior(np.array([[[0, 1], [1, 0]], [[1, 0], [1, 0]]], dtype=i64)),
        "categorical_float_onehot": lambda: lm("categorical", 3).update_posterior(np.array([[0.0, 1.0, 0.0]])),
        "categorical_wrong_last_dim": lambda: lm("categorical", 3).update_posterior(np.array([[0, 1], [1, 0]], dtype=i64)),
        "categorical_index_equals_degree": lambda: lm("categorical", 3).update_posterior(np.array([0, 3, 1], dtype=i64), onehot=False),
        "categorical_index_negative": lambda: lm("categorical", 3).update_posterior(np.array([0, -1, 1], dtype=i64), onehot=False),
        "categorical_index_float": lambda: lm("categorical", 3).update_posterior(np.array([0.0, 1.0]), onehot=False),
        "categorical_index_ok": lambda: lm("categorical", 3).update_posterior(np.array([0, 2, 1], dtype=i64), onehot=False),
        "categorical_index_scalar_ok": lambda: lm("categorical", 3).update_posterior(2, onehot=False),
        "categorical_index_scalar_too_large": lambda: lm("categorical", 3).update_posterior(3, onehot=False),
        "categorical_scalar_as_onehot": lambda: lm("categorical", 3).update_posterior(2),
        "categorical_ctor_zero_degree": lambda: lm("categorical", 0),
        "categorical_ctor_float_degree": lambda: lm("categorical", 3.0),
        "categorical_h0_alpha_vec_nonpos": lambda: lm("categorical", 3, h0_alpha_vec=np.array([1.0, 0.0, 1.0])),
        "categorical_h0_alpha_vec_scalar_ok": lambda: lm("categorical", 3, h0_alpha_vec=2),
        "categorical_bad_loss_estimate": lambda: lm("categorical", 3).estimate_params("abs"),
        "categorical_bad_loss_prediction": lambda: lm("categorical", 3).make_prediction("abs"),
        "categorical_gen_theta_not_sum_1": lambda: mods["categorical"].GenModel(3, theta_vec=np.array([0.5, 0.5, 0.5])),
        "categorical_gen_theta_wrong_dim": lambda: mods["categorical"].GenModel(3, theta_vec=np.array([0.5, 0.5])),
        "poisson_negative": lambda: lm("poisson").update_posterior(np.array([3, -1, 0], dtype=i64)),
        "poisson_float_array": lambda: lm("poisson").update_posterior(np.array([1.0, 2.0])),
        "poisson_scalar_negative": lambda: lm("poisson").update_posterior(-1),
        "poisson_scalar_ok": lambda: lm("poisson").update_posterior(4),
        "poisson_pred_float": lambda: lm("poisson").pred_and_update(2.0),
        "poisson_h0_alpha_zero": lambda: lm("poisson", h0_alpha=0.0),
        "poisson_bad_loss_estimate": lambda: lm("poisson").estimate_params("L1"),
        "poisson_bad_loss_prediction": lambda: lm("poisson").make_prediction("L1"),
        "poisson_gen_lambda_nonpos": lambda: mods["poisson"].GenModel(lambda_=0.0),
        "exponential_zero": lambda: lm("exponential").update_posterior(np.array([1.0, 0.0, 2.0])),
        "exponential_negative_zero": lambda: lm("exponential").update_posterior(np.array([1.0, -0.0, 2.0])),
        "exponential_nan": lambda: lm("exponential").update_posterior(np.array([1.0, np.nan, 2.0])),
        "exponential_negative": lambda: lm("exponential").update_posterior(np.array([1.0, -2.0])),
        "exponential_int_array_ok": lambda: lm("exponential").update_posterior(np.array([1, 2, 3], dtype=i64)),
        "exponential_int_array_zero": lambda: lm("exponential").update_posterior(np.array([1, 0, 3], dtype=i64)),
        "exponential_list": lambda: lm("exponential").update_posterior([1.0, 2.0]),
        "exponential_scalar_zero": lambda: lm("exponential").update_posterior(0.0),
        "exponential_scalar_int_ok": lambda: lm("exponential").update_posterior(3),
        "exponential_h0_beta_nonpos": lambda: lm("exponential", h0_beta=0.0),
        "exponential_bad_loss_estimate": lambda: lm("exponential").estimate_params("L1"),
        "exponential_bad_loss_prediction": lambda: lm("exponential").make_prediction("L1"),
        "exponential_interval_out_of_range": lambda: lm("exponential").estimate_interval(-0.1),
        "normal_int_array_ok": lambda: lm("normal").update_posterior(np.array([1, 2, 3], dtype=i64)),
        "normal_bool_array": lambda: lm("normal").update_posterior(np.array([True, False])),
        "normal_complex_array": lambda: lm("normal").update_posterior(np.array([1.0 + 0j])),
        "normal_list": lambda: lm("normal").update_posterior([1.0, 2.0]),
        "normal_scalar_int_ok": lambda: lm("normal").update_posterior(3),
        "normal_pred_string": lambda: lm("normal").pred_and_update("1.0"),
        "normal_h0_kappa_nonpos": lambda: lm("normal", h0_kappa=0.0),
        "normal_h0_alpha_nonpos": lambda: lm("normal", h0_alpha=-1.0),
        "normal_h0_m_list": lambda: lm("normal", h0_m=[0.0]),
        "normal_bad_loss_estimate": lambda: lm("normal").estimate_params("L1"),
        "normal_bad_loss_prediction": lambda: lm("normal").make_prediction("L1"),
        "normal_gen_tau_nonpos": lambda: mods["normal"].GenModel(tau=0.0),
        "normal_gen_float_size": lambda: mods["normal"].GenModel().gen_sample(10.0),
    }
