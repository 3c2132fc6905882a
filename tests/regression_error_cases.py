"""The boundary cases of linearregression / autoregressive whose outcome (exception class name, or None) is recorded
from the reference in tests/golden/linreg_errors.json and ar_errors.json and replayed against the drop-in
(TEST INFRASTRUCTURE ONLY).  ``mod`` is the model package; ``prepare`` is applied to every LearnModel made."""
import numpy as np


def _maker(mod, prepare):
    def lm(*a, **k):
        m = mod.LearnModel(*a, **k)
        if prepare is not None:
            prepare(m)
        return m
    return lm


def linreg_error_cases(mod, prepare=None):
    lm = _maker(mod, prepare)
    return {
        "ctor_float_degree": lambda: lm(2.0),
        "ctor_zero_degree": lambda: lm(0),
        "h0_mu_vec_wrong_dim": lambda: lm(2, h0_mu_vec=np.zeros(3)),
        "h0_mu_vec_list": lambda: lm(2, h0_mu_vec=[0.0, 0.0]),
        "h0_lambda_mat_not_pd": lambda: lm(2, h0_lambda_mat=np.array([[1.0, 2.0], [2.0, 1.0]])),
        "h0_lambda_mat_wrong_dim": lambda: lm(2, h0_lambda_mat=np.eye(3)),
        "h0_alpha_nonpos": lambda: lm(2, h0_alpha=0.0),
        "h0_beta_negative": lambda: lm(2, h0_beta=-1.0),
        "h0_alpha_int_ok": lambda: lm(2, h0_alpha=3),
        "x_wrong_last_dim": lambda: lm(2).update_posterior(np.zeros((5, 3)), np.zeros(5)),
        "x_not_ndarray": lambda: lm(2).update_posterior([[0.0, 1.0]], np.zeros(1)),
        "y_shape_mismatch": lambda: lm(2).update_posterior(np.zeros((5, 2)), np.zeros(4)),
        "y_list": lambda: lm(2).update_posterior(np.zeros((5, 2)), [0.0] * 5),
        "y_scalar_with_rows": lambda: lm(2).update_posterior(np.zeros((5, 2)), 1.0),
        "y_scalar_one_row_ok": lambda: lm(2).update_posterior(np.ones(2), 1.0),
        "x_int_ok": lambda: lm(2).update_posterior(np.arange(10).reshape(5, 2), np.arange(5)),
        "x_3d_ok": lambda: lm(2).update_posterior(np.ones((3, 4, 2)), np.ones((3, 4))),
        "bad_loss_estimate": lambda: lm(2).estimate_params("L1"),
        "bad_loss_prediction": lambda: lm(2).make_prediction("L1"),
        "pred_dist_wrong_dim": lambda: lm(2).calc_pred_dist(np.zeros((4, 3))),
        "pred_dist_complex": lambda: lm(2).calc_pred_dist(np.zeros((4, 2), dtype=complex)),
        "gen_sample_nothing": lambda: mod.GenModel(2).gen_sample(),
        "gen_sample_float_size": lambda: mod.GenModel(2).gen_sample(3.0),
        "gen_theta_wrong_dim": lambda: mod.GenModel(2, theta_vec=np.zeros(3)),
        "gen_tau_nonpos": lambda: mod.GenModel(2, tau=0.0),
    }


def ar_error_cases(mod, prepare=None):
    lm = _maker(mod, prepare)
    return {
        "ctor_float_degree": lambda: lm(2.0),
        "ctor_negative_degree": lambda: lm(-1),
        "ctor_zero_degree_ok": lambda: lm(0).update_posterior(np.arange(4.0)),
        "h0_mu_vec_wrong_dim": lambda: lm(2, h0_mu_vec=np.zeros(2)),
        "h0_lambda_mat_not_pd": lambda: lm(1, h0_lambda_mat=np.array([[1.0, 2.0], [2.0, 1.0]])),
        "h0_lambda_mat_wrong_dim": lambda: lm(2, h0_lambda_mat=np.eye(2)),
        "h0_alpha_nonpos": lambda: lm(2, h0_alpha=0.0),
        "h0_beta_negative": lambda: lm(2, h0_beta=-1.0),
        "x_too_short": lambda: lm(3).update_posterior(np.zeros(3)),
        "x_2d": lambda: lm(1).update_posterior(np.zeros((5, 1))),
        "x_list": lambda: lm(1).update_posterior([0.0, 1.0, 2.0]),
        "x_int_ok": lambda: lm(1).update_posterior(np.arange(6)),
        "padding_unknown_ok": lambda: lm(1).update_posterior(np.arange(6.0), padding="ones"),
        "bad_loss_estimate": lambda: lm(2).estimate_params("L1"),
        "bad_loss_prediction": lambda: lm(2).make_prediction("L1"),
        "pred_dist_wrong_len": lambda: lm(2).calc_pred_dist(np.zeros(3)),
        "pred_and_update_wrong_len": lambda: lm(2).pred_and_update(np.zeros(2)),
        "interval_out_of_range": lambda: lm(2).predict_interval(1.5),
        "gen_sample_float_length": lambda: mod.GenModel(2).gen_sample(3.0),
        "gen_initial_values_wrong_len": lambda: mod.GenModel(2).gen_sample(5, initial_values=np.zeros(3)),
        "gen_theta_wrong_dim": lambda: mod.GenModel(2, theta_vec=np.zeros(2)),
    }
