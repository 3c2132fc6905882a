"""Input validators of the boundary (the subset the GMM/HMM path uses).

Behavioural restatement of ``bayesml/_check.py`` (reference file:line in each docstring): each
validator returns the (possibly float-cast) value or raises ``exc(name + message)``.  Written
around two predicates (`_is_int`, `_is_real`) instead of the reference's copy-per-function style.
"""
import numpy as np

_EPSILON = np.sqrt(np.finfo(np.float64).eps)


# What each sample validator below says when it refuses (the one source of these messages): the scalar conjugate models check the TYPE of an array on the host
# by these rules and leave the VALUE check to the data pass on the device (include/expfam.h: `bad`).
SAMPLE_MSG = {
    "nonneg_ints": " must be int or a numpy.ndarray whose dtype is int. Its values must be non-negative (including 0).",
    "ints_of_01": " must be int or a numpy.ndarray whose dtype is int. Its values must be 0 or 1.",
    "onehot_vecs": " must be a numpy.ndarray whose dtype is int and whose last axis constitutes one-hot vectors.",
    "pos_floats": " must be float or a numpy.ndarray. Its values must be positive (not including 0)",
    "floats": " must be float or a numpy.ndarray.",
}


def _is_int(v):
    return np.issubdtype(type(v), np.integer)


def _is_real(v):
    return _is_int(v) or np.issubdtype(type(v), np.floating)


def _arr_kind(v):
    """'i' / 'f' for integer / floating ndarrays, None for anything else (lists, complex, ...)."""
    if type(v) is not np.ndarray:
        return None
    if np.issubdtype(v.dtype, np.integer):
        return "i"
    if np.issubdtype(v.dtype, np.floating):
        return "f"
    return None


def pos_int(val, name, exc):
    """_check.py:28-32 — Python/NumPy integers > 0 only (floats such as 2.0 are rejected)."""
    if _is_int(val) and val > 0:
        return val
    raise exc(name + " must be int. Its value must be positive (not including 0).")


def pos_float(val, name, exc):
    """_check.py:19-26 — positive real scalar (integers are cast to float)."""
    if _is_real(val) and val > 0.0:
        return float(val) if _is_int(val) else val
    raise exc(name + " must be positive (not including 0.0).")


def floats(val, name, exc):
    """_check.py:163-173 — real scalar or real ndarray (ints are cast); no sign condition."""
    if _is_real(val):
        return float(val) if _is_int(val) else val
    kind = _arr_kind(val)
    if kind is not None:
        return val.astype(float) if kind == "i" else val
    raise exc(name + SAMPLE_MSG["floats"])


def pos_floats(val, name, exc):
    """_check.py:175-185 — positive real scalar or positive real ndarray (ints are cast)."""
    if _is_real(val) and val > 0.0:
        return float(val) if _is_int(val) else val
    kind = _arr_kind(val)
    if kind is not None and np.all(val > 0):
        return val.astype(float) if kind == "i" else val
    raise exc(name + SAMPLE_MSG["pos_floats"])


def float_vec(val, name, exc):
    """_check.py:187-193 — 1-dimensional real ndarray."""
    kind = _arr_kind(val)
    if kind is not None and val.ndim == 1:
        return val.astype(float) if kind == "i" else val
    raise exc(name + " must be a 1-dimensional numpy.ndarray.")


def float_vecs(val, name, exc):
    """_check.py:203-209 — real ndarray with ndim >= 1."""
    kind = _arr_kind(val)
    if kind is not None and val.ndim >= 1:
        return val.astype(float) if kind == "i" else val
    raise exc(name + " must be a numpy.ndarray whose ndim >= 1.")


def float_vec_sum_1(val, name, exc):
    """_check.py:219-225 — 1-dimensional real ndarray summing to 1 within sqrt(eps)."""
    kind = _arr_kind(val)
    if kind is not None and val.ndim == 1 and abs(val.sum() - 1.0) <= _EPSILON:
        return val.astype(float) if kind == "i" else val
    raise exc(name + " must be a 1-dimensional numpy.ndarray, and the sum of its elements must equal to 1.")


def float_vecs_sum_1(val, name, exc):
    """_check.py:227-233 — real ndarray whose last axis sums to 1 within sqrt(eps)."""
    kind = _arr_kind(val)
    if kind is not None and val.ndim >= 1 and np.all(np.abs(np.sum(val, axis=-1) - 1.0) <= _EPSILON):
        return val.astype(float) if kind == "i" else val
    raise exc(name + " must be a numpy.ndarray whose ndim >= 1, and the sum along the last dimension must equal to 1.")


def pos_def_sym_mats(val, name, exc):
    """_check.py:140-154 — stack of symmetric (np.allclose) positive-definite (batched Cholesky) matrices."""
    ok = (type(val) is np.ndarray and val.ndim >= 2 and val.shape[-1] == val.shape[-2]
          and np.allclose(val, np.swapaxes(val, -1, -2)))
    if not ok:
        raise exc(name + " must be a symmetric 2-dimensional numpy.ndarray.")
    try:
        np.linalg.cholesky(val)
    except np.linalg.LinAlgError:
        raise exc(name + " must be a positive definite symmetric 2-dimensional numpy.ndarray.") from None
    return val


def pos_def_sym_mat(val, name, exc):
    """_check.py:124-138 — one symmetric (np.allclose) positive-definite (Cholesky) matrix."""
    ok = type(val) is np.ndarray and val.ndim == 2 and val.shape[0] == val.shape[1] and np.allclose(val, val.T)
    if not ok:
        raise exc(name + " must be a symmetric 2-dimensional numpy.ndarray.")
    try:
        np.linalg.cholesky(val)
    except np.linalg.LinAlgError:
        raise exc(name + " must be a positive definite symmetric 2-dimensional numpy.ndarray.") from None
    return val


def shape_consistency(val, val_name, correct, correct_name, exc):
    """_check.py:268-272."""
    if val != correct:
        raise exc(f"{val_name} must coincide with {correct_name}: {val_name} = {val}, {correct_name} = {correct}")


def nonneg_int(val, name, exc):
    """_check.py:34-38 — Python/NumPy integers >= 0 only."""
    if _is_int(val) and val >= 0:
        return val
    raise exc(name + " must be int. Its value must be non-negative (including 0).")


def float_in_closed01(val, name, exc):
    """_check.py:10-17 — real scalar in [0, 1] (integers are cast to float)."""
    if _is_real(val) and 0.0 <= val <= 1.0:
        return float(val) if _is_int(val) else val
    raise exc(name + " must be in [0,1].")


def float_(val, name, exc):
    """_check.py:156-161 — real scalar (integers are cast to float); no sign condition."""
    if _is_real(val):
        return float(val) if _is_int(val) else val
    raise exc(name + " must be a scalar.")


def nonneg_ints(val, name, exc):
    """_check.py:40-48 — integer scalar >= 0, or integer ndarray whose values are all >= 0."""
    if _is_int(val) and val >= 0:
        return val
    if _arr_kind(val) == "i" and np.all(val >= 0):
        return val
    raise exc(name + SAMPLE_MSG["nonneg_ints"])


def int_of_01(val, name, exc):
    """_check.py:91-95 — the integer 0 or 1 (bool and floats are rejected)."""
    if _is_int(val) and (val == 0 or val == 1):
        return val
    raise exc(name + " must be int. Its value must be 0 or 1.")


def ints_of_01(val, name, exc):
    """_check.py:97-105 — the integer 0 or 1, or an integer ndarray of zeros and ones."""
    if _is_int(val) and (val == 0 or val == 1):
        return val
    if _arr_kind(val) == "i" and np.all(val >= 0) and np.all(val <= 1):
        return val
    raise exc(name + SAMPLE_MSG["ints_of_01"])


def onehot_vec(val, name, exc):
    """_check.py:250-254 — 1-dimensional integer ndarray, no negative entry, entries summing to 1."""
    if _arr_kind(val) == "i" and val.ndim == 1 and np.all(val >= 0) and val.sum() == 1:
        return val
    raise exc(name + " must be a one-hot vector (1-dimensional ndarray) whose dtype must be int.")


def onehot_vecs(val, name, exc):
    """_check.py:256-260 — integer ndarray (ndim >= 1), no negative entry, every last-axis sum equal to 1."""
    if _arr_kind(val) == "i" and val.ndim >= 1 and np.all(val >= 0) and np.all(val.sum(axis=-1) == 1):
        return val
    raise exc(name + SAMPLE_MSG["onehot_vecs"])


def sample_kind(val):
    """'i' / 'f' for an integer / floating ndarray or torch tensor (bool, complex and everything else: None)."""
    if type(val) is np.ndarray:
        return _arr_kind(val)
    try:
        import torch
    except ImportError:      # pragma: no cover
        return None
    if isinstance(val, torch.Tensor):
        if val.dtype.is_floating_point:
            return "f"
        if val.dtype != torch.bool and not val.dtype.is_complex:
            return "i"
    return None


def pos_ints(val, name, exc):
    """_check.py:50-58 — integer scalar > 0, or integer ndarray whose values are all > 0."""
    if _is_int(val) and val > 0:
        return val
    if _arr_kind(val) == "i" and np.all(val > 0):
        return val
    raise exc(name + " must be int or a numpy.ndarray whose dtype is int. Its values must be positive (not including 0).")


def ints(val, name, exc):
    """_check.py:60-66 — integer scalar or integer ndarray; no sign condition."""
    if _is_int(val) or _arr_kind(val) == "i":
        return val
    raise exc(name + " must be int or a numpy.ndarray whose dtype is int.")


def nonneg_float_vec(val, name, exc):
    """_check.py:195-201 — 1-dimensional real ndarray without a negative entry."""
    kind = _arr_kind(val)
    if kind is not None and val.ndim == 1 and np.all(val >= 0):
        return val.astype(float) if kind == "i" else val
    raise exc(name + " must be a 1-dimensional numpy.ndarray. Its values must be non-negative (including 0).")
