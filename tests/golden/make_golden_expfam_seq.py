#!/usr/bin/env python3
"""Golden fixtures for ``pred_and_update_sequence`` of the scalar conjugate models, produced by the REFERENCE (build
container only):

    MPLBACKEND=Agg python tests/golden/make_golden_expfam_seq.py

writes tests/golden/expfam_seq_<family>.npz (categorical: expfam_seq_categorical_d3.npz and _d300.npz, where the loop is
walked in the index form and in the one-hot form; ``pred_01_onehot`` holds the latter's one-hot predictions, and its rows,
checked equal to the index form's, are stored once as ``pred_squared``).  Per family and
per start (``prior``: the default h0; ``post``: after ``update_posterior`` of 500 earlier values) the file keeps, under
``<start>_``:

    x               300 observations of the seeded recipe
    hn0, hn1        hn_* before the loop and after it, in the order of get_hn_params()
    pred_<loss>     the loop's ``pred_and_update(x[i], loss)`` for every loss that returns numbers (None -> NaN)
    nats            ``-log(_calc_pred_density(x[i]))`` before each update
    nats_err        |nats - the same formula in mpmath at the reference's own parameters|: the reference's own error, which
                    the tests add to their bound
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
os.environ.setdefault("MPLBACKEND", "Agg")

from bayesml import bernoulli, categorical, exponential, normal, poisson          # noqa: E402
import expfam_seq_oracle as orc                                      # noqa: E402
from bayesml_amd import _expseq as xs                                # noqa: E402

N, N_EARLIER = 300, 500
FAMILIES = {"bernoulli": (bernoulli, xs.BERNOULLI, ("squared", "0-1", "abs", "KL")),
            "poisson": (poisson, xs.POISSON, ("squared", "0-1", "abs")),
            "exponential": (exponential, xs.EXPONENTIAL, ("squared", "0-1", "abs")),
            "normal": (normal, xs.NORMAL, ("squared", "0-1", "abs"))}


def walk(mod, fam, losses, earlier, x):
    out = {"x": x}
    for loss in losses:
        m = mod.LearnModel()
        if earlier is not None:
            m.update_posterior(earlier)
        out["hn0"] = np.array(list(m.get_hn_params().values()), dtype=np.float64)
        preds, nats, err = [], [], []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for i, v in enumerate(x):
                v = v.item()
                m.calc_pred_dist()
                p = [float(t) for t in m.get_p_params().values()]
                nats.append(-np.log(m._calc_pred_density(v)))
                if fam == xs.POISSON:
                    exact, _ = orc.nats_mp(fam, p, v, beta_i=m.hn_beta)
                elif fam == xs.NORMAL:
                    exact, _ = orc.nats_mp(fam, (m.p_mu, m.p_nu, m.p_lambda), v)
                elif fam == xs.EXPONENTIAL:
                    exact, _ = orc.nats_mp(fam, (m.p_kappa, m.p_lambda), v)
                else:
                    exact, _ = orc.nats_mp(fam, p, v)
                err.append(abs(float(nats[-1] - exact)))
                r = m.pred_and_update(v, loss)
                preds.append(np.nan if r is None else r)
        out["pred_" + loss.replace("-", "")] = np.array(preds)
        out["nats"], out["nats_err"] = np.array(nats, dtype=np.float64), np.array(err)
        out["hn1"] = np.array(list(m.get_hn_params().values()), dtype=np.float64)
    return out


def walk_categorical(degree, earlier, x):
    out = {"x": x}
    eye = np.eye(degree, dtype=int)
    for onehot in (False, True):
        for loss in ("squared", "0-1"):
            m = categorical.LearnModel(degree)
            if earlier is not None:
                m.update_posterior(earlier, onehot=False)
            out["hn0"] = m.hn_alpha_vec.copy()
            preds, nats = [], []
            for v in x:
                m.calc_pred_dist()
                nats.append(-np.log(m._calc_pred_density(int(v))))
                preds.append(np.copy(m.pred_and_update(eye[v] if onehot else int(v), loss, onehot)))
            if loss == "squared" and onehot:          # the rows do not depend on the input form: stored once
                assert np.array_equal(np.array(preds), out["pred_squared"])
            else:
                out["pred_" + loss.replace("-", "") + ("_onehot" if onehot else "")] = np.array(preds)
            out["nats"], out["hn1"] = np.array(nats), m.hn_alpha_vec.copy()
    return out


def main():
    for degree in (3, 300):
        data = {}
        for start, seed in (("prior", 11), ("post", 12)):
            earlier = orc.cat_sample(degree, N_EARLIER, seed=seed + 100) if start == "post" else None
            for k, v in walk_categorical(degree, earlier, orc.cat_sample(degree, N, seed=seed)).items():
                data[f"{start}_{k}"] = v
        path = os.path.join(HERE, f"expfam_seq_categorical_d{degree}.npz")
        np.savez_compressed(path, **data)
        print(path, os.path.getsize(path))
    for name, (mod, fam, losses) in FAMILIES.items():
        data = {}
        for start, seed in (("prior", 11), ("post", 12)):
            earlier = orc.sample(fam, N_EARLIER, seed=seed + 100) if start == "post" else None
            for k, v in walk(mod, fam, losses, earlier, orc.sample(fam, N, seed=seed)).items():
                data[f"{start}_{k}"] = v
        path = os.path.join(HERE, f"expfam_seq_{name}.npz")
        np.savez_compressed(path, **data)
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
