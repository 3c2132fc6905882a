"""``metatree.GenModel`` / ``LearnModel``: drop-in for ``bayesml/metatree/_metatree.py`` (cited below as ``ref:<lines>``).

The reference keeps a forest of Python ``_Node`` trees and updates it by boolean-mask recursion, once per tree and once
per node (ref:1729-1770).  Here the posterior forest lives in flat tables (``_mtree.FlatForest`` and the state tables
``g``, ``post``, ``lml``, ``lcm``, ``prob``) and ``update_posterior`` is the batch form of DESIGN.md section 4i:
``mtree_route`` finds every row's stop node in every tree, ``mtree_reduce`` sums y per stop node without floating-point
atomics, ``mtree_sweep`` folds, mixes and weights bottom-up in one launch.  ``predict`` and its relatives are
``mtree_predict``.  ``hn_metatree_list`` is a property that materialises ``_Node`` trees from the tables on demand; a list
given to a setter or to the constructor is flattened into them.  The tables stay on the host until an update or a
prediction needs the engine, so setters and getters work without a GPU.

``SubModel=linearregression`` puts a Bayesian linear regression over all continuous features into every node
(``sub_constants={'c_degree': c_dim_continuous}``, at most ``_mtree.LR_MAX_DEGREE``; anything else is an
``EngineLimitError`` that says what to pass): ``mtree_reduce_x`` sorts every tree's rows by stop node and forms one X'X per
node on the f64 MFMA, the sweep factors it per node.

``alg_type='MTMCMC'`` / ``'REMTMCMC'`` learn the tree structure from the data: every chain's proposal grows level by level on
the device (``_mtgrow.Grower``, include/mtgrow.h) in a complete tree of (C^(c_max_depth + 1) - 1) / (C - 1) slots (at most
``_mtree.MAX_NODES``; at most ``_mtree.MAX_TREES`` chains; ``EngineLimitError`` beyond), is scored by the same route, reduce
and sweep, and ``mtgrow_accept`` applies the Metropolis-Hastings test; the lists, the counts, g_max and the exchanges are host
scalars.  Their random numbers are ADDRESSED Philox tables (``_mtgrow.node_table`` / ``aux_table``), not the reference's
depth-first stream: a ``seed`` reproduces this package's chain and the reference's distribution, not the reference's chain.

Out of scope, with an error that names it: plotting (``NotImplementedError``).  MTRF grows its forest with
scikit-learn on the host, as the reference does; scikit-learn is imported in that path only.

``GenModel`` is host NumPy.
"""
from __future__ import annotations

import warnings

import numpy as np

from .. import _check, _mtree, base
from .. import bernoulli, categorical, exponential, linearregression, normal, poisson
from .._engine import EngineLimitError
from .._exceptions import CriteriaError, DataFormatError, ParameterFormatError, ResultWarning

MODELS = {bernoulli, categorical, normal, linearregression, poisson, exponential}
DISCRETE_MODELS = {bernoulli, categorical, poisson}
CONTINUOUS_MODELS = {normal, linearregression, exponential}
CLF_MODELS = {bernoulli, categorical}
REG_MODELS = {normal, linearregression, exponential, poisson}
THRESHOLD_TYPES = {"even", "random"}
_FAMILY = {bernoulli: _mtree.BERNOULLI, categorical: _mtree.CATEGORICAL, poisson: _mtree.POISSON,
           exponential: _mtree.EXPONENTIAL, normal: _mtree.NORMAL, linearregression: _mtree.LINREG}
_SUBMODEL_MSG = "SubModel must be bernoulli, categoricalpoisson, normal, exponential, or linearregression."
_LR_MSG = ("SubModel=linearregression regresses y on all continuous features: pass sub_constants={'c_degree': "
           "c_dim_continuous} with c_dim_continuous >= 1 (an intercept is a column of ones in x_continuous)")
_INT_VECS_MSG = " must be a numpy.ndarray whose ndim >= 1 and dtype is int. Its values must be non-negative (including 0)."


class _Node:
    """The reference's node (ref:82-110): same constructor and public attributes (its two private scratch attributes, which
    only its own recursions use, are left out)."""

    def __init__(self, depth, k_candidates=None, h_g=0.5, k=None, sub_model=None, children=None, ranges=None,
                 thresholds=None, leaf=False, map_leaf=False, log_children_marginal_likelihood=None,
                 log_marginal_likelihood=None):
        self.depth = depth
        self.children = children
        self.k_candidates = k_candidates
        self.h_g = h_g
        self.k = k
        self.sub_model = sub_model
        self.ranges = ranges
        self.thresholds = thresholds
        self.leaf = leaf
        self.map_leaf = map_leaf
        self.log_children_marginal_likelihood = log_children_marginal_likelihood
        self.log_marginal_likelihood = log_marginal_likelihood


def _check_lr_constants(c_dim_continuous, sub_constants):
    """SubModel=linearregression: the reference hands x_continuous as it is to every node's learner (ref:1772-1774), so its
    c_degree is c_dim_continuous.  A missing or different c_degree (a TypeError, or a DataFormatError at the first sample,
    in the reference) is refused here, as is a degree beyond the engine's one-tile Gram pass."""
    degree = sub_constants.get("c_degree") if isinstance(sub_constants, dict) else None
    if degree is None:
        raise EngineLimitError(_LR_MSG + "; sub_constants has no 'c_degree'")
    if degree != c_dim_continuous:
        raise EngineLimitError(_LR_MSG + f"; got c_degree = {degree} and c_dim_continuous = {c_dim_continuous}")
    _mtree.check_lr_degree(int(degree))


def _check_constants(self, c_dim_continuous, c_dim_categorical, c_max_depth, c_num_children_vec, c_num_assignment_vec,
                     c_ranges, SubModel, sub_constants):
    """The constants block that GenModel and LearnModel share (ref:196-242, 1178-1224)."""
    self.c_dim_continuous = _check.nonneg_int(c_dim_continuous, "c_dim_continuous", ParameterFormatError)
    self.c_dim_categorical = _check.nonneg_int(c_dim_categorical, "c_dim_categorical", ParameterFormatError)
    _check.pos_int(self.c_dim_continuous + self.c_dim_categorical, "c_dim_continuous+c_dim_categorical", ParameterFormatError)
    self.c_dim_features = self.c_dim_continuous + self.c_dim_categorical
    self.c_max_depth = _check.pos_int(c_max_depth, "c_max_depth", ParameterFormatError)
    _check.pos_ints(c_num_children_vec, "c_num_children_vec", ParameterFormatError)
    if np.any(c_num_children_vec < 2):
        raise ParameterFormatError("All the elements of c_num_children_vec must be greater than or equal to 2: "
                                   f"c_num_children_vec={c_num_children_vec}.")
    self.c_num_children_vec = np.ones(self.c_dim_features, dtype=int) * 2
    self.c_num_children_vec[:] = c_num_children_vec
    self.c_num_assignment_vec = -np.ones(self.c_dim_features, dtype=int)
    if c_num_assignment_vec is not None:
        _check.ints(c_num_assignment_vec, "c_num_assignment_vec", ParameterFormatError)
        if np.all(c_num_assignment_vec == 0):
            raise ParameterFormatError("At least one element of c_num_assignment_vec must be non-zero: "
                                       f"c_num_assignment_vec={c_num_assignment_vec}.")
        self.c_num_assignment_vec[:] = c_num_assignment_vec
    self.c_ranges = np.zeros([self.c_dim_continuous, 2])
    self.c_ranges[:, 0] -= 3
    self.c_ranges[:, 1] += 3
    if c_ranges is not None:
        _check.float_vecs(c_ranges, "c_ranges", ParameterFormatError)
        self.c_ranges[:] = c_ranges
        if np.any(self.c_ranges[:, 0] > self.c_ranges[:, 1]):
            raise ParameterFormatError("self.c_ranges[:,1] must be greater than or equal to self.c_ranges[:,0]")
    if SubModel not in MODELS:
        raise ParameterFormatError(_SUBMODEL_MSG)
    if SubModel is linearregression:
        _check_lr_constants(self.c_dim_continuous, sub_constants)
    self.SubModel = SubModel
    self._root_k_candidates = []
    for i in range(self.c_dim_features):
        self._root_k_candidates.extend([i] * (1 if self.c_num_assignment_vec[i] < 0 else self.c_num_assignment_vec[i]))


def _child_candidates(node_candidates, k, c_num_assignment_vec):
    out = list(node_candidates)
    if c_num_assignment_vec[k] > 0:
        out.remove(k)
    return out


def _rename(params, to):
    """ref:1426-1434: keys of any of the three prefixes are accepted."""
    out = {}
    for key, val in params.items():
        for frm in ("h0_", "hn_", "h_"):
            if key.startswith(frm) and frm != to:
                key = key.replace(frm, to, 1)
                break
        out[key] = val
    return out


def _child_index(node, c_dim_continuous, x_continuous, x_categorical):
    """The child a single row goes to (None where it matches none)."""
    n_children = len(node.children)
    if node.k < c_dim_continuous:
        x, t = x_continuous[node.k], node.thresholds
        if x < t[1]:
            return 0
        if t[n_children - 1] <= x:
            return n_children - 1
        for i in range(1, n_children - 1):
            if t[i] <= x < t[i + 1]:
                return i
        return None
    v = int(x_categorical[node.k - c_dim_continuous])
    return v if 0 <= v < n_children else None


class GenModel(base.Generative):
    """Data-generating model and its prior (ref:112-1087; plotting is out of scope)."""

    def __init__(self, c_dim_continuous, c_dim_categorical, c_max_depth=2, c_num_children_vec=2, c_num_assignment_vec=None,
                 c_ranges=None, SubModel=bernoulli, sub_constants={}, root=None, h_k_weight_vec=None, h_g=0.5,
                 sub_h_params={}, h_metatree_list=[], h_metatree_prob_vec=None, seed=None):
        _check_constants(self, c_dim_continuous, c_dim_categorical, c_max_depth, c_num_children_vec, c_num_assignment_vec,
                         c_ranges, SubModel, sub_constants)
        self.sub_constants = self.SubModel.GenModel(**sub_constants).get_constants()
        self.rng = np.random.default_rng(seed)
        self.h_k_weight_vec = np.ones(self.c_dim_features)
        self.h_g = 0.5
        self.sub_h_params = {}
        self.h_metatree_list = []
        self.h_metatree_prob_vec = None
        self.set_h_params(h_k_weight_vec, h_g, sub_h_params, h_metatree_list, h_metatree_prob_vec)
        self.root = _Node(0, self._root_k_candidates, self.h_g, sub_model=self._new_sub(), ranges=self.c_ranges, leaf=True)
        self.set_params(root)

    def _new_sub(self):
        return self.SubModel.GenModel(seed=self.rng, **self.sub_constants, **self.sub_h_params)

    def get_constants(self):
        return {"c_dim_continuous": self.c_dim_continuous, "c_dim_categorical": self.c_dim_categorical,
                "c_num_children_vec": self.c_num_children_vec, "c_max_depth": self.c_max_depth,
                "c_num_assignment_vec": self.c_num_assignment_vec, "c_ranges": self.c_ranges,
                "sub_constants": self.sub_constants}

    # ---- tree plumbing ---------------------------------------------------------------------------------------------------
    def _num_children(self, node):
        return int(self.c_num_children_vec[node.k])

    def _make_children(self, node):
        """ref:306-328: missing children are created, existing ones get the parent's candidates and ranges."""
        cand = _child_candidates(node.k_candidates, node.k, self.c_num_assignment_vec)
        node.leaf = False
        for i in range(self._num_children(node)):
            if node.children[i] is None:
                node.children[i] = _Node(node.depth + 1, k_candidates=cand, h_g=self.h_g, sub_model=self._new_sub(),
                                         ranges=np.array(node.ranges))
            else:
                node.children[i].k_candidates = cand
                node.children[i].ranges = np.array(node.ranges)
            if node.thresholds is not None:
                node.children[i].ranges[node.k, 0] = node.thresholds[i]
                node.children[i].ranges[node.k, 1] = node.thresholds[i + 1]

    def _gen_thresholds(self, node, threshold_type):
        n, (lo, hi) = self._num_children(node), node.ranges[node.k]
        node.thresholds = np.empty(n + 1)
        if threshold_type == "random":
            steps = self.rng.dirichlet(np.ones(n)) * (hi - lo)
            node.thresholds[0] = lo
            for i in range(n):
                node.thresholds[i + 1] = node.thresholds[i] + steps[i]
        if threshold_type == "even":
            node.thresholds[:] = np.linspace(lo, hi, n + 1)

    @staticmethod
    def _prior_of(h_node):
        try:
            return h_node.sub_model.get_h_params()
        except AttributeError:
            return h_node.sub_model.get_hn_params()

    def _gen_params(self, node, h_node, feature_fix, threshold_fix, threshold_type):
        """ref:341-377: the draws in the reference's order (the split coin, the feature, the thresholds, then the children
        left to right; a leaf draws its sub-model's parameter)."""
        g = self.h_g if h_node is None else h_node.h_g
        node.h_g = 0 if node.depth == self.c_max_depth else g
        if h_node is None:
            node.sub_model.set_h_params(**self.sub_h_params)
        else:
            node.sub_model.set_h_params(*self._prior_of(h_node).values())
        if node.depth == self.c_max_depth or not node.k_candidates or self.rng.random() > g:
            node.sub_model.gen_params()
            node.leaf = True
            return
        if h_node is None:
            fresh = node.k is None
            if not feature_fix or fresh:
                w = self.h_k_weight_vec[node.k_candidates]
                node.k = self.rng.choice(node.k_candidates, p=w / w.sum())
                node.children = [None] * self._num_children(node)
            if node.k < self.c_dim_continuous and (not threshold_fix or fresh):
                self._gen_thresholds(node, threshold_type)
            else:
                node.thresholds = None
        else:
            node.k = h_node.k
            node.children = [None] * self._num_children(node)
            node.thresholds = np.array(h_node.thresholds) if node.k < self.c_dim_continuous else None
        self._make_children(node)
        for i in range(self._num_children(node)):
            self._gen_params(node.children[i], None if h_node is None else h_node.children[i], feature_fix, threshold_fix,
                             threshold_type)

    def _gen_params_fixed_tree(self, node, threshold_fix, threshold_type):
        """ref:379-401: shape and features stay, thresholds (unless fixed) and leaf parameters are drawn."""
        node.h_g = 0 if node.depth == self.c_max_depth else self.h_g
        node.sub_model.set_h_params(**self.sub_h_params)
        if node.leaf:
            node.sub_model.gen_params()
            return
        if node.k < self.c_dim_continuous and not threshold_fix:
            self._gen_thresholds(node, threshold_type)
        else:
            node.thresholds = None
        cand = _child_candidates(node.k_candidates, node.k, self.c_num_assignment_vec)
        for i in range(self._num_children(node)):
            child = node.children[i]
            if child is not None:
                child.k_candidates = cand
                child.ranges = np.array(node.ranges)
                if node.thresholds is not None:
                    child.ranges[node.k, 0] = node.thresholds[i]
                    child.ranges[node.k, 1] = node.thresholds[i + 1]
                self._gen_params_fixed_tree(child, threshold_fix, threshold_type)

    def _set_params(self, node, orig):
        """ref:403-422."""
        if orig.leaf:
            try:
                sub_params = orig.sub_model.get_params()
            except AttributeError:
                try:
                    sub_params = orig.sub_model.estimate_params(loss="0-1", dict_out=True)
                except Exception:
                    sub_params = orig.sub_model.estimate_params(dict_out=True)
            node.sub_model.set_params(**sub_params)
            if node.depth == self.c_max_depth:
                node.h_g = 0
            node.leaf = True
            return
        node.k = orig.k
        node.children = [None] * self._num_children(node)
        node.thresholds = np.array(orig.thresholds) if node.k < self.c_dim_continuous else None
        self._make_children(node)
        for i in range(self._num_children(node)):
            self._set_params(node.children[i], orig.children[i])

    def _walk(self, fn, node):
        fn(node)
        if not node.leaf:
            for child in node.children:
                self._walk(fn, child)

    def _set_h_tree(self, node, orig):
        """ref:504-530: superpose ``orig`` on ``node``; where ``orig`` is None the defaults go to everything below."""
        if orig is None:
            node.h_g = 0 if node.depth == self.c_max_depth else self.h_g
            node.sub_model.set_h_params(**self.sub_h_params)
            if not node.leaf:
                for child in node.children:
                    self._set_h_tree(child, None)
            return
        node.h_g = 0 if node.depth == self.c_max_depth else orig.h_g
        node.sub_model.set_h_params(*self._prior_of(orig).values())
        if orig.leaf or node.depth == self.c_max_depth:
            node.leaf = True
            node.h_g = 0
            return
        node.k = orig.k
        node.children = [None] * self._num_children(node)
        node.thresholds = np.array(orig.thresholds) if node.k < self.c_dim_continuous else None
        self._make_children(node)
        for i in range(self._num_children(node)):
            self._set_h_tree(node.children[i], orig.children[i])

    # ---- the API ----------------------------------------------------------------------------------------------------------
    def set_h_params(self, h_k_weight_vec=None, h_g=None, sub_h_params=None, h_metatree_list=None, h_metatree_prob_vec=None):
        if h_k_weight_vec is not None:
            _check.nonneg_float_vec(h_k_weight_vec, "h_k_weight_vec", ParameterFormatError)
            _check.shape_consistency(h_k_weight_vec.shape[0], "h_k_weight_vec.shape[0]", self.c_dim_features,
                                     "self.c_dim_features", ParameterFormatError)
            self.h_k_weight_vec[:] = h_k_weight_vec
        if h_g is not None:
            self.h_g = _check.float_in_closed01(h_g, "h_g", ParameterFormatError)
            for h_root in self.h_metatree_list:
                self._walk(lambda nd: setattr(nd, "h_g", 0 if nd.depth == self.c_max_depth else self.h_g), h_root)
        if sub_h_params is not None:
            self.sub_h_params = self.SubModel.GenModel(seed=self.rng, **self.sub_constants,
                                                       **_rename(sub_h_params, "h_")).get_h_params()
            for h_root in self.h_metatree_list:
                self._walk(lambda nd: nd.sub_model.set_h_params(**self.sub_h_params), h_root)
        if h_metatree_list is not None:
            if not isinstance(h_metatree_list, list):
                raise ParameterFormatError("h_metatree_list must be a list")
            for h_root in h_metatree_list:
                if type(h_root) is not _Node:
                    raise ParameterFormatError("all elements of h_metatree_list must be instances of metatree._Node or empty")
            diff = len(h_metatree_list) - len(self.h_metatree_list)
            if diff < 0:
                del self.h_metatree_list[diff:]
            for _ in range(max(diff, 0)):
                self.h_metatree_list.append(_Node(0, self._root_k_candidates, self.h_g, sub_model=self._new_sub(),
                                                  ranges=self.c_ranges))
            for mine, given in zip(self.h_metatree_list, h_metatree_list):
                self._set_h_tree(mine, given)
            if h_metatree_prob_vec is not None:
                self.h_metatree_prob_vec = np.array(_check.float_vec_sum_1(h_metatree_prob_vec, "h_metatree_prob_vec",
                                                                           ParameterFormatError))
            elif h_metatree_list:
                self.h_metatree_prob_vec = np.ones(len(self.h_metatree_list)) / len(self.h_metatree_list)
            else:
                self.h_metatree_prob_vec = None
        elif h_metatree_prob_vec is not None:
            self.h_metatree_prob_vec = np.array(_check.float_vec_sum_1(h_metatree_prob_vec, "h_metatree_prob_vec",
                                                                       ParameterFormatError))
        _check_prob_vec(self.h_metatree_prob_vec, self.h_metatree_list, "h_metatree")
        return self

    def get_h_params(self):
        return {"h_k_weight_vec": self.h_k_weight_vec, "h_g": self.h_g, "sub_h_params": self.sub_h_params,
                "h_metatree_list": self.h_metatree_list, "h_metatree_prob_vec": self.h_metatree_prob_vec}

    def gen_params(self, feature_fix=False, threshold_fix=False, tree_fix=False, threshold_type="even"):
        if threshold_type not in THRESHOLD_TYPES:
            raise ParameterFormatError('threshold_type must be "even" or "random"')
        if feature_fix:
            if tree_fix:
                self._gen_params_fixed_tree(self.root, threshold_fix, threshold_type)
            else:
                warnings.warn("If feature_fix=True, tree will be generated according to "
                              "self.h_g not any element of self.h_metatree_list.", ResultWarning)
                self._gen_params(self.root, None, True, threshold_fix, threshold_type)
        else:
            if threshold_fix or tree_fix:
                warnings.warn("If feature_fix=False, threshold and tree cannot be fixed.", ResultWarning)
            h_root = self.rng.choice(self.h_metatree_list, p=self.h_metatree_prob_vec) if self.h_metatree_list else None
            self._gen_params(self.root, h_root, False, False, threshold_type)
        return self

    def set_params(self, root=None):
        if root is not None:
            if type(root) is not _Node:
                raise ParameterFormatError("root must be an instance of metatree._Node")
            self._set_params(self.root, root)
        return self

    def get_params(self):
        return {"root": self.root}

    def _check_categorical(self, x_categorical):
        if not (type(x_categorical) is np.ndarray and np.issubdtype(x_categorical.dtype, np.integer)
                and x_categorical.ndim >= 1 and np.all(x_categorical >= 0)):
            raise DataFormatError("x_categorical" + _INT_VECS_MSG)
        _check.shape_consistency(x_categorical.shape[-1], "x_categorical.shape[-1]", self.c_dim_categorical,
                                 "self.c_dim_categorical", ParameterFormatError)
        x_categorical = x_categorical.reshape(-1, self.c_dim_categorical)
        _check_cat_max(x_categorical, self.c_num_children_vec, self.c_dim_continuous)
        return x_categorical

    def _draw_continuous(self, sample_size):
        x = np.empty([sample_size, self.c_dim_continuous], dtype=float)
        for i in range(self.c_dim_continuous):
            x[:, i] = (self.c_ranges[i, 1] - self.c_ranges[i, 0]) * self.rng.random(sample_size) + self.c_ranges[i, 0]
        return x

    def _draw_categorical(self, sample_size):
        x = np.empty([sample_size, self.c_dim_categorical], dtype=int)
        for i in range(self.c_dim_categorical):
            x[:, i] = self.rng.choice(self.c_num_children_vec[self.c_dim_continuous + i], sample_size)
        return x

    def gen_sample(self, sample_size=None, x_continuous=None, x_categorical=None):
        """ref:747-857: features that are not given are drawn (continuous first), then y row by row from the leaf each row
        reaches."""
        if x_continuous is not None:
            _check.float_vecs(x_continuous, "x_continuous", DataFormatError)
            _check.shape_consistency(x_continuous.shape[-1], "x_continuous.shape[-1]", self.c_dim_continuous,
                                     "self.c_dim_continuous", ParameterFormatError)
            x_continuous = x_continuous.reshape(-1, self.c_dim_continuous)
            sample_size = x_continuous.shape[0]
            if x_categorical is not None:
                x_categorical = self._check_categorical(x_categorical)
                _check.shape_consistency(x_categorical.shape[0], "x_categorical.shape[0]", x_continuous.shape[0],
                                         "x_continuous.shape[0]", ParameterFormatError)
            else:
                x_categorical = self._draw_categorical(sample_size)
        elif x_categorical is not None:
            x_categorical = self._check_categorical(x_categorical)
            sample_size = x_categorical.shape[0]
            x_continuous = self._draw_continuous(sample_size)
        elif sample_size is not None:
            sample_size = _check.pos_int(sample_size, "sample_size", DataFormatError)
            x_continuous = self._draw_continuous(sample_size)
            x_categorical = self._draw_categorical(sample_size)
        else:
            raise DataFormatError("Either of sample_size, x_continuous, and x_categorical must be given as a input.")
        y = np.empty(sample_size, dtype=int if self.SubModel in DISCRETE_MODELS else float)
        for i in range(sample_size):
            node = self.root
            while not node.leaf:
                node = node.children[_child_index(node, self.c_dim_continuous, x_continuous[i], x_categorical[i])]
            if self.SubModel is linearregression:        # ref:426-428: the row's continuous features are the regressors
                y[i] = np.ravel(node.sub_model.gen_sample(sample_size=1, x=x_continuous[i])[1])[0]
            elif self.SubModel is categorical:
                y[i] = np.ravel(node.sub_model.gen_sample(sample_size=1, onehot=False))[0]
            else:
                y[i] = np.ravel(node.sub_model.gen_sample(sample_size=1))[0]
        return x_continuous, x_categorical, y

    def save_sample(self, filename, sample_size, x_continuous=None, x_categorical=None):
        x_continuous, x_categorical, y = self.gen_sample(sample_size, x_continuous, x_categorical)
        np.savez_compressed(filename, x_continuous=x_continuous, x_categorical=x_categorical, y=y)

    def visualize_model(self, filename=None, format=None, sample_size=100, x_continuous=None, x_categorical=None):
        _check.pos_int(sample_size, "sample_size", DataFormatError)
        raise NotImplementedError(_mtree.PLOT_MSG)


def _check_prob_vec(prob_vec, tree_list, name):
    """ref:645-658."""
    if type(prob_vec) is np.ndarray:
        if prob_vec.shape[0] != len(tree_list):
            raise ParameterFormatError(f"Length of {name}_list and dimension of {name}_prob_vec must be the same.")
    elif prob_vec is None:
        if len(tree_list) > 0:
            raise ParameterFormatError(f"Length of {name}_list must be zero when self.{name}_prob_vec is None.")
    else:
        raise ParameterFormatError(f"self.{name}_prob_vec must be None or a numpy.ndarray.")


def _check_cat_max(x_categorical, c_num_children_vec, c_dim_continuous):
    for i in range(x_categorical.shape[1]):
        if x_categorical[:, i].max() >= c_num_children_vec[c_dim_continuous + i]:
            raise _cat_error(i, c_num_children_vec, c_dim_continuous)


def _cat_error(i, c_num_children_vec, c_dim_continuous):
    return DataFormatError(f"x_categorical[:,{i}].max() must smaller than self.c_num_children_vec[{c_dim_continuous + i}]: "
                           f"{c_num_children_vec[c_dim_continuous + i]}")


class _Forest:
    """A forest as tables on the host: the structure and the state (g, post, lml, lcm per node; prob per tree)."""

    def __init__(self, flat, state):
        self.flat, self.state = flat, state

    def copy(self):
        return _Forest(self.flat, {k: np.array(v) for k, v in self.state.items()})


class LearnModel(base.Posterior, base.PredictiveMixin):
    """Posterior and predictive distribution (ref:1089-3625).  Positional parameters are the reference's; keyword-only
    ``device`` selects the GPU.  Samples may be NumPy arrays or torch tensors.

    The engine, and with it the GPU, is first needed by ``update_posterior``, ``pred_and_update`` or a prediction on a
    non-empty forest; without a GPU those calls raise ``EngineUnavailableError``."""

    _mtree_pass_factory = None        # private test seam (tests/fake_metatree_engine.py)

    def __init__(self, c_dim_continuous, c_dim_categorical, c_max_depth=2, c_num_children_vec=2, c_num_assignment_vec=None,
                 c_ranges=None, SubModel=bernoulli, sub_constants={}, h0_k_weight_vec=None, h0_g=0.5, sub_h0_params={},
                 h0_metatree_list=[], h0_metatree_prob_vec=None, *, device=None):
        _check_constants(self, c_dim_continuous, c_dim_categorical, c_max_depth, c_num_children_vec, c_num_assignment_vec,
                         c_ranges, SubModel, sub_constants)
        self.sub_constants = self.SubModel.LearnModel(**sub_constants).get_constants()
        self._family = _FAMILY[self.SubModel]
        self._degree = int(self.sub_constants.get("c_degree", 0))
        _mtree.check_limits(0, 0, int(self.c_num_children_vec.max()), 0, self._degree)
        self._device = device
        self._engine = None
        self._h0 = None               # _Forest or None
        self._hn = None               # _Forest or None; while the engine lives, its state is the engine's
        self._p_x = None
        self._last_map = None
        self._mcmc_trace = None       # per step of the last MTMCMC / REMTMCMC fit: what mtgrow_accept returned, the exchanges

        self.h0_k_weight_vec = np.ones(self.c_dim_features)
        self.h0_g = 0.5
        self.sub_h0_params = {}
        self.hn_k_weight_vec = np.ones(self.c_dim_features)
        self.hn_g = 0.5
        self.sub_hn_params = {}
        self._p_n = 0
        self.set_h0_params(h0_k_weight_vec, h0_g, sub_h0_params, h0_metatree_list, h0_metatree_prob_vec)

    # ---- the posterior vector of a node and the scalar learners -----------------------------------------------------------
    def _new_sub(self):
        return self.SubModel.LearnModel(**self.sub_constants, **self.sub_h0_params)

    def _post_of(self, sub):
        f = self._family
        if f == _mtree.CATEGORICAL:
            return np.array(sub.hn_alpha_vec, dtype=float)
        if f == _mtree.LINREG:        # [mu | upper triangle of Lambda, row-major | alpha | beta | n]
            lam = np.asarray(sub.hn_lambda_mat, dtype=float)
            return np.concatenate([np.asarray(sub.hn_mu_vec, dtype=float), lam[np.triu_indices(self._degree)],
                                   [sub.hn_alpha, sub.hn_beta, sub._n]])
        if f == _mtree.NORMAL:
            return np.array([sub.hn_m, sub.hn_kappa, sub.hn_alpha, sub.hn_beta, sub._n], dtype=float)
        if f == _mtree.POISSON:
            return np.array([sub.hn_alpha, sub.hn_beta, sub._sum_log_factorial], dtype=float)
        return np.array([sub.hn_alpha, sub.hn_beta], dtype=float)

    def _sub_from(self, vec, which="hn"):
        """A scalar learner whose ``which`` hyperparameters are the post vector ``vec``."""
        sub = self._new_sub()
        f = self._family
        if f == _mtree.LINREG:
            mu, lam, alpha, beta, n = self._lr_parts(vec)
            vals = (mu, lam, alpha, beta)
        else:
            vals = ((np.array(vec),) if f == _mtree.CATEGORICAL
                    else tuple(float(v) for v in vec[:4 if f == _mtree.NORMAL else 2]))
        if which == "h0":
            sub.set_h0_params(*vals)
            return sub
        sub.set_hn_params(*vals)
        if f == _mtree.LINREG:
            sub._n = int(n) if float(n).is_integer() else n
        elif f == _mtree.NORMAL:
            sub._n = int(vec[4]) if float(vec[4]).is_integer() else vec[4]
        elif f == _mtree.POISSON:
            sub._sum_log_factorial = float(vec[2])
        return sub

    def _lr_parts(self, vec):
        """(mu, symmetric Lambda, alpha, beta, n) of a linear-regression post vector."""
        D = self._degree
        T = D * (D + 1) // 2
        lam = np.zeros((D, D))
        lam[np.triu_indices(D)] = vec[D:D + T]
        lam = lam + np.triu(lam, 1).T
        return np.array(vec[:D], dtype=float), lam, float(vec[D + T]), float(vec[D + T + 1]), vec[D + T + 2]

    def _prior_vec(self):
        """The engine's h0 vector: the sub-model's prior in the layout of a post vector."""
        sub = self._new_sub()
        return self._post_of(sub)

    def _default_post(self):
        return self._post_of(self._new_sub().set_hn_params(**self.sub_hn_params))

    # ---- flat tables <-> _Node trees -------------------------------------------------------------------------------------
    def _flatten(self, roots, prob, getter, default_g):
        """Breadth-first tables of a list of ``_Node`` trees.  ``getter(sub_model)`` gives a node's hyperparameters as the
        reference's copying recursions read them (ref:1301-1306, 1352-1357); a node without a sub-model takes the
        defaults.  g is 0 at the maximal depth, where every node is a leaf."""
        tree_off, feat, child0, nchild, thr_off, depth, thr, g, post, lml, lcm = [0], [], [], [], [], [], [], [], [], [], []
        default_post = self._default_post()
        for root in roots:
            order, base_i = [(root, 0.0)], len(feat)
            i = 0
            while i < len(order):
                node, own_lcm = order[i]
                leaf = bool(node.leaf) or node.depth == self.c_max_depth or node.children is None
                if node.sub_model is None:
                    post.append(default_post)
                else:
                    tmp = self._new_sub()
                    tmp.set_hn_params(*getter(node.sub_model).values())
                    post.append(self._post_of(tmp))
                g.append(0.0 if node.depth == self.c_max_depth else float(default_g if node.h_g is None else node.h_g))
                depth.append(node.depth)
                lml.append(np.nan)
                lcm.append(own_lcm)
                if leaf:
                    feat.append(-1)
                    child0.append(0)
                    nchild.append(0)
                    thr_off.append(-1)
                else:
                    k = int(node.k)
                    n_children = int(self.c_num_children_vec[k])
                    feat.append(k)
                    child0.append(base_i + len(order))
                    nchild.append(n_children)
                    if k < self.c_dim_continuous:
                        thr_off.append(len(thr))
                        thr.extend(np.asarray(node.thresholds, dtype=float)[:n_children + 1])
                    else:
                        thr_off.append(-1)
                    order.extend((node.children[c], 0.0) for c in range(n_children))
                i += 1
            tree_off.append(len(feat))
        flat = _mtree.FlatForest(np.array(tree_off, np.int32), np.array(feat, np.int32), np.array(child0, np.int32),
                                 np.array(nchild, np.int32), np.array(thr_off, np.int32), np.array(depth, np.int32),
                                 np.array(thr, np.float64))
        _mtree.check_limits(flat.n_trees, flat.max_tree_nodes, flat.max_children, flat.max_depth, self._degree)
        state = dict(g=np.array(g, float), post=np.array(post, float).reshape(len(g), -1), lml=np.array(lml, float),
                     lcm=np.array(lcm, float), prob=np.array(prob, float))
        return _Forest(flat, state)

    def _materialise(self, forest, which):
        """The ``_Node`` trees of a forest (fresh objects: host work proportional to the nodes)."""
        if forest is None:
            return []
        fl, st = forest.flat, forest.state
        roots = []
        nodes = [None] * fl.n_nodes
        for b in range(fl.n_trees):
            lo, hi = int(fl.tree_off[b]), int(fl.tree_off[b + 1])
            nodes[lo] = _Node(0, list(self._root_k_candidates), ranges=np.array(self.c_ranges))
            for v in range(lo, hi):
                node = nodes[v]
                node.h_g = float(st["g"][v])
                node.sub_model = self._sub_from(st["post"][v], which)
                node.log_marginal_likelihood = None if np.isnan(st["lml"][v]) else float(st["lml"][v])
                if fl.feat[v] < 0:
                    node.leaf = True
                    node.log_children_marginal_likelihood = np.zeros(2)
                    continue
                k, n_children, c0 = int(fl.feat[v]), int(fl.nchild[v]), int(fl.child0[v])
                node.k = k
                node.leaf = False
                node.thresholds = (np.array(fl.thr[fl.thr_off[v]:fl.thr_off[v] + n_children + 1])
                                   if k < self.c_dim_continuous else None)
                node.log_children_marginal_likelihood = np.array(st["lcm"][c0:c0 + n_children])
                cand = _child_candidates(node.k_candidates, k, self.c_num_assignment_vec)
                node.children = []
                for c in range(n_children):
                    child = _Node(node.depth + 1, cand, ranges=np.array(node.ranges))
                    if node.thresholds is not None:
                        child.ranges[k, 0] = node.thresholds[c]
                        child.ranges[k, 1] = node.thresholds[c + 1]
                    nodes[c0 + c] = child
                    node.children.append(child)
            roots.append(nodes[lo])
        return roots

    # ---- the engine ---------------------------------------------------------------------------------------------------------
    def _hn_forest(self):
        """The posterior forest with its current state on the host (None when empty)."""
        if self._hn is not None and self._engine is not None:
            self._hn.state = self._engine.get_state()
        return self._hn

    def _set_hn(self, forest):
        if self._engine is not None:
            self._engine.close()
        self._engine = None
        self._hn = forest

    def _eng(self):
        if self._engine is None:
            cat_card = self.c_num_children_vec[self.c_dim_continuous:]
            args = (self._hn.flat, self._family, self._degree, self.c_dim_continuous, self.c_dim_categorical, cat_card,
                    self._prior_vec())
            make = self._mtree_pass_factory
            self._engine = make(*args) if make is not None else _mtree.MtreePass(*args, device=self._device)
            self._engine.set_state(self._hn.state)
        return self._engine

    def __getstate__(self):
        """The tables come back from the device; the engine, the kept rows and the SubModel module (by name) are left out."""
        self._hn_forest()
        state = dict(self.__dict__)
        state["_engine"] = None
        state["_p_x"] = None
        state["SubModel"] = self.SubModel.__name__
        return state

    def __setstate__(self, state):
        import importlib
        self.__dict__.update(state)
        self.SubModel = importlib.import_module(state["SubModel"])

    @property
    def h0_metatree_list(self):
        return self._materialise(self._h0, "h0")

    @property
    def h0_metatree_prob_vec(self):
        return None if self._h0 is None else self._h0.state["prob"]

    @property
    def hn_metatree_list(self):
        """The posterior forest as the reference's ``_Node`` trees (fresh copies), ``[]`` when empty."""
        return self._materialise(self._hn_forest(), "hn")

    @property
    def hn_metatree_prob_vec(self):
        forest = self._hn_forest()
        return None if forest is None else forest.state["prob"]

    def get_constants(self):
        return {"c_dim_continuous": self.c_dim_continuous, "c_dim_categorical": self.c_dim_categorical,
                "c_num_children_vec": self.c_num_children_vec, "c_max_depth": self.c_max_depth,
                "c_num_assignment_vec": self.c_num_assignment_vec, "c_ranges": self.c_ranges,
                "sub_constants": self.sub_constants}

    # ---- hyperparameters ---------------------------------------------------------------------------------------------------
    def _set_forest(self, which, forest, tree_list, prob_vec, g, getter):
        """The list / prob_vec part that set_h0_params and set_hn_params share (ref:1442-1508, 1590-1656).  Returns the
        new forest (or None)."""
        name = f"{which}_metatree"
        if tree_list is not None:
            if not isinstance(tree_list, list):
                raise ParameterFormatError(f"{name}_list must be a list")
            for root in tree_list:
                if type(root) is not _Node:
                    raise ParameterFormatError(f"all elements of {name}_list must be instances of metatree._Node or empty")
            if prob_vec is not None:
                prob = np.array(_check.float_vec_sum_1(prob_vec, f"{name}_prob_vec", ParameterFormatError))
            else:
                prob = np.ones(len(tree_list)) / len(tree_list) if tree_list else None
            _check_prob_vec(prob, tree_list, name)
            return self._flatten(tree_list, prob, getter, g) if tree_list else None
        if prob_vec is not None:
            prob = np.array(_check.float_vec_sum_1(prob_vec, f"{name}_prob_vec", ParameterFormatError))
            _check_prob_vec(prob, [None] * (0 if forest is None else forest.flat.n_trees), name)
            forest = forest.copy()
            forest.state["prob"] = prob
        return forest

    def _fill(self, forest, g=None, post=None):
        """ref:1281-1291, 1332-1342: a new default for every node of an existing forest."""
        if forest is None:
            return
        if g is not None:
            forest.state["g"][:] = np.where(forest.flat.depth == self.c_max_depth, 0.0, g)
        if post is not None:
            forest.state["post"][:] = post

    def set_h0_params(self, h0_k_weight_vec=None, h0_g=None, sub_h0_params=None, h0_metatree_list=None,
                      h0_metatree_prob_vec=None):
        if h0_k_weight_vec is not None:
            _check.nonneg_float_vec(h0_k_weight_vec, "h0_k_weight_vec", ParameterFormatError)
            _check.shape_consistency(h0_k_weight_vec.shape[0], "h0_k_weight_vec.shape[0]", self.c_dim_features,
                                     "self.c_dim_features", ParameterFormatError)
            self.h0_k_weight_vec[:] = h0_k_weight_vec
        if h0_g is not None:
            self.h0_g = _check.float_in_closed01(h0_g, "h0_g", ParameterFormatError)
            self._fill(self._h0, g=self.h0_g)
        if sub_h0_params is not None:
            self.sub_h0_params = self.SubModel.LearnModel(**self.sub_constants,
                                                          **_rename(sub_h0_params, "h0_")).get_h0_params()
            self._fill(self._h0, post=self._prior_vec())

        def getter(sub):
            try:
                return sub.get_h_params()
            except AttributeError:
                return sub.get_h0_params()
        self._h0 = self._set_forest("h0", self._h0, h0_metatree_list, h0_metatree_prob_vec, self.h0_g, getter)
        self.reset_hn_params()
        return self

    def get_h0_params(self):
        return {"h0_k_weight_vec": self.h0_k_weight_vec, "h0_g": self.h0_g, "sub_h0_params": self.sub_h0_params,
                "h0_metatree_list": self.h0_metatree_list, "h0_metatree_prob_vec": self.h0_metatree_prob_vec}

    def set_hn_params(self, hn_k_weight_vec=None, hn_g=None, sub_hn_params=None, hn_metatree_list=None,
                      hn_metatree_prob_vec=None):
        if hn_k_weight_vec is not None:
            _check.nonneg_float_vec(hn_k_weight_vec, "hn_k_weight_vec", ParameterFormatError)
            _check.shape_consistency(hn_k_weight_vec.shape[0], "hn_k_weight_vec.shape[0]", self.c_dim_features,
                                     "self.c_dim_features", ParameterFormatError)
            self.hn_k_weight_vec[:] = hn_k_weight_vec
        forest = self._hn_forest()
        if hn_g is not None:
            self.hn_g = _check.float_in_closed01(hn_g, "hn_g", ParameterFormatError)
            self._fill(forest, g=self.hn_g)
        if sub_hn_params is not None:
            self.sub_hn_params = self._new_sub().set_hn_params(**_rename(sub_hn_params, "hn_")).get_hn_params()
            self._fill(forest, post=self._default_post())

        def getter(sub):
            try:
                return sub.get_h_params()
            except AttributeError:
                return sub.get_hn_params()
        self._set_hn(self._set_forest("hn", forest, hn_metatree_list, hn_metatree_prob_vec, self.hn_g, getter))
        self._p_x, self._p_n = None, 1          # (the reference ends with calc_pred_dist of one row of zeros, ref:1658-1660)
        return self

    def get_hn_params(self):
        return {"hn_k_weight_vec": self.hn_k_weight_vec, "hn_g": self.hn_g, "sub_hn_params": self.sub_hn_params,
                "hn_metatree_list": self.hn_metatree_list, "hn_metatree_prob_vec": self.hn_metatree_prob_vec}

    # ---- the sample --------------------------------------------------------------------------------------------------------
    def _check_sample_x(self, x_continuous, x_categorical):
        """Types and shapes on the host (ref:1956-2010); the categorical VALUES are checked by the route pass (``bad``).
        Returns the matrices as [n, dim] (None where the dimension is 0) and n."""
        xc = xk = None
        if self.c_dim_continuous > 0:
            if _check.sample_kind(x_continuous) is None or x_continuous.ndim < 1:
                raise DataFormatError("x_continuous must be a numpy.ndarray whose ndim >= 1.")
            _check.shape_consistency(x_continuous.shape[-1], "x_continuous.shape[-1]", self.c_dim_continuous,
                                     "self.c_dim_continuous", ParameterFormatError)
            xc = x_continuous.reshape(-1, self.c_dim_continuous)
        if self.c_dim_categorical > 0:
            if _check.sample_kind(x_categorical) != "i" or x_categorical.ndim < 1:
                raise DataFormatError("x_categorical" + _INT_VECS_MSG)
            _check.shape_consistency(x_categorical.shape[-1], "x_categorical.shape[-1]", self.c_dim_categorical,
                                     "self.c_dim_categorical", ParameterFormatError)
            xk = x_categorical.reshape(-1, self.c_dim_categorical)
        if xc is not None and xk is not None:
            _check.shape_consistency(xc.shape[0], "x_continuous.shape[0]", xk.shape[0], "x_categorical.shape[0]",
                                     ParameterFormatError)
        return xc, xk, int((xc if xc is not None else xk).shape[0])

    def _check_sample_y(self, y, xc=None):
        """The sub-model's own sample check (ref:2012-2017), on whatever holds y; returns it flat.  Linear regression checks
        y against the rows of x_continuous (``xc``, [n, c_dim_continuous]); without ``xc`` (ref:3507-3508) y alone."""
        kind = _check.sample_kind(y)
        f = self._family
        if f == _mtree.LINREG:
            if xc is not None:
                return self._new_sub()._check_sample(xc, y)[1]
            if kind is None:
                raise DataFormatError("y" + _check.SAMPLE_MSG["floats"])
            y = y.reshape(-1)
            return y if kind == "f" else (y.astype(float) if type(y) is np.ndarray else y.double())
        if kind is None or (f <= _mtree.POISSON and kind != "i"):
            key = {_mtree.BERNOULLI: "ints_of_01", _mtree.CATEGORICAL: "nonneg_ints", _mtree.POISSON: "nonneg_ints",
                   _mtree.EXPONENTIAL: "pos_floats", _mtree.NORMAL: "floats"}[f]
            raise DataFormatError("x" + _check.SAMPLE_MSG[key])
        y = y.reshape(-1)
        if y.shape[0] == 0:
            return y
        lo, hi = y.min(), y.max()
        if f == _mtree.BERNOULLI and (lo < 0 or hi > 1):
            raise DataFormatError("x" + _check.SAMPLE_MSG["ints_of_01"])
        if f in (_mtree.CATEGORICAL, _mtree.POISSON) and lo < 0:
            raise DataFormatError("x" + _check.SAMPLE_MSG["nonneg_ints"])
        if f == _mtree.CATEGORICAL and hi >= self._degree:
            raise DataFormatError("np.max(x) must be smaller than self.c_degree: "
                                  f"np.max(x) = {int(hi)}, self.c_degree = {self._degree}")
        if f == _mtree.EXPONENTIAL and not lo > 0:
            raise DataFormatError("x" + _check.SAMPLE_MSG["pos_floats"])
        return y

    def _raise_bad(self, xk):
        """The reference's message for a categorical value outside its range (ref:1972-1977), after ``bad > 0``."""
        lo = xk.min(0)
        lo = lo.values if hasattr(lo, "values") else lo
        if bool((lo < 0).any()):
            raise DataFormatError("x_categorical" + _INT_VECS_MSG)
        hi = xk.max(0)
        hi = hi.values if hasattr(hi, "values") else hi
        for i in range(self.c_dim_categorical):
            if int(hi[i]) >= self.c_num_children_vec[self.c_dim_continuous + i]:
                raise _cat_error(i, self.c_num_children_vec, self.c_dim_continuous)
        raise DataFormatError("x_categorical" + _INT_VECS_MSG)

    def _check_values(self, xk):
        """ref:1965, 1972-1977: every categorical value in 0 .. c_num_children_vec - 1, on a host array or a tensor (two
        column reductions; a tensor on the device costs one read-back)."""
        if xk is None or xk.shape[0] == 0:
            return
        lo, hi = xk.min(0), xk.max(0)
        lo, hi = (lo.values, hi.values) if hasattr(lo, "values") else (lo, hi)
        card = self.c_num_children_vec[self.c_dim_continuous:]
        if bool((lo < 0).any()) or any(int(hi[i]) >= card[i] for i in range(self.c_dim_categorical)):
            self._raise_bad(xk)

    # ---- learning ----------------------------------------------------------------------------------------------------------
    def _copy_sklearn_tree(self, tree):
        """ref:1681-1723: an inner node of the scikit-learn tree stays inner while features remain to assign; the
        threshold sits between the node's range ends; a leaf has h_g = 0 (children start from h0_g, the root from hn_g)."""
        root = _Node(0, list(self._root_k_candidates), self.hn_g, ranges=np.array(self.c_ranges))
        stack = [(root, 0)]
        while stack:
            node, nid = stack.pop()
            if tree.children_left[nid] == -1 or not node.k_candidates:
                node.h_g = 0.0
                node.leaf = True
                continue
            k = node.k = int(tree.feature[nid])
            if k < self.c_dim_continuous:
                node.thresholds = np.array([node.ranges[k, 0], tree.threshold[nid], node.ranges[k, 1]])
            cand = _child_candidates(node.k_candidates, k, self.c_num_assignment_vec)
            node.children = []
            for side, cid in enumerate((tree.children_left[nid], tree.children_right[nid])):
                child = _Node(node.depth + 1, cand, h_g=self.h0_g, ranges=np.array(node.ranges))
                if node.thresholds is not None:
                    child.ranges[k, 1 - side] = node.thresholds[1]
                node.children.append(child)
                stack.append((child, int(cid)))
        return root

    def _same_tree(self, a, b):
        """ref:1819-1843."""
        if a.leaf or b.leaf:
            return bool(a.leaf and b.leaf)
        if a.k != b.k or (a.k < self.c_dim_continuous and not np.allclose(a.thresholds, b.thresholds)):
            return False
        return all(self._same_tree(ca, cb) for ca, cb in zip(a.children, b.children))

    def _merge_trees(self, trees, prob):
        """ref:1845-1856: a tree equal to a later one hands its probability to that one."""
        trees = list(trees)
        for i in range(len(trees)):
            for j in range(i + 1, len(trees)):
                if self._same_tree(trees[i], trees[j]):
                    trees[i] = None
                    prob[j] += prob[i]
                    prob[i] = -1
                    break
        return [t for t in trees if t is not None], prob[prob > -0.5]

    def _mtrf(self, xc, xk, y, n_estimators=100, **kwargs):
        """ref:1858-1921: the forest is grown by scikit-learn on the host, from float64 features, continuous first."""
        if np.any(self.c_num_children_vec != 2):
            raise ParameterFormatError("MTRF is supported only when all the elements of c_num_children_vec is 2.")
        from sklearn.ensemble import RandomForestClassifier, RandomForestRegressor
        make = RandomForestClassifier if self.SubModel in CLF_MODELS else RandomForestRegressor
        forest = make(n_estimators=n_estimators, max_depth=self.c_max_depth, **kwargs)

        def host(a):
            return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
        x = np.empty([y.shape[0], self.c_dim_features])
        if xc is not None:
            x[:, :self.c_dim_continuous] = host(xc)
        if xk is not None:
            x[:, self.c_dim_continuous:] = host(xk)
        forest.fit(x, host(y))
        trees = [self._copy_sklearn_tree(est.tree_) for est in forest.estimators_]
        trees, prob = self._merge_trees(trees, np.ones(n_estimators) / n_estimators)
        return self._flatten(trees, prob, None, self.hn_g)

    # ---- MTMCMC / REMTMCMC (ref:2029-2665) --------------------------------------------------------------------------------
    # The chains run on the growth engine (``_mtgrow.Grower``): a chain's tree is a table over the
    # ``cap`` slots of the complete C-ary tree in heap order, the host keeps the lists, the counts, g_max and the exchanges.
    # Random numbers are ADDRESSED (``_mtgrow.node_table`` / ``aux_table``), not streamed: a seed reproduces this package's
    # chain and the reference's distribution, not the reference's chain.
    def _mcmc_checks(self, threshold_type, num_chains=None):
        """The preconditions the two algorithms share, with the reference's texts (ref:2044-2075, 2151-2184)."""
        if np.any(self.c_num_children_vec != self.c_num_children_vec[0]):
            raise ParameterFormatError("MTMCMC is supported only when all the elements of self.c_num_children_vec are the same. "
                                       f"self.c_num_children_vec = {self.c_num_children_vec}.")
        if np.any(self.c_num_assignment_vec > 0):
            raise ParameterFormatError("MTMCMC is supported only when all the elements of self.c_num_assignment_vec are not "
                                       f"positive. self.c_num_assignment_vec = {self.c_num_assignment_vec}.")
        if not np.allclose(self.h0_k_weight_vec, self.h0_k_weight_vec[0]):
            raise ParameterFormatError("MTMCMC is supported only when all the elements of self.h0_k_weight_vec are the same. "
                                       f"self.h0_k_weight_vec = {self.h0_k_weight_vec}.")
        if num_chains is not None:
            _check.pos_int(num_chains, "num_chains", ParameterFormatError)
        if threshold_type not in {"1d_kmeans", "sample_midpoint"}:
            raise ParameterFormatError('threshold_type must be "1d_kmeans" or "sample_midpoint".')

    def _grower(self, alg_type, num_chains, threshold_type, xc, xk, y):
        """The growth engine of the installed factory: the real one, or the seam's ``grower`` (a factory without one cannot
        run the chains)."""
        from .. import _mtgrow
        C = int(self.c_num_children_vec[0])
        _mtgrow.capacity(C, self.c_max_depth, num_chains)          # EngineLimitError before anything is built
        args = (self._family, self._degree, self.c_dim_continuous, self.c_dim_categorical,
                self.c_num_children_vec[self.c_dim_continuous:], C, self.c_max_depth, self._prior_vec(), self._default_post(),
                self.hn_g, self.h0_g, threshold_type, num_chains, xc, xk, y)
        make = self._mtree_pass_factory
        if make is None:
            return _mtgrow.Grower(*args, device=self._device)
        grower = getattr(make, "grower", None)
        if grower is None:
            raise NotImplementedError(f"alg_type='{alg_type}' needs an engine that grows trees (bayesml_amd._mtgrow); the "
                                      "installed engine factory has none")
        return grower(*args)

    @staticmethod
    def _mcmc_key(seed):
        """The Philox key of a fit: ``seed`` itself where it is a non-negative integer below 2^64, fresh entropy for None,
        and anything else NumPy seeds a generator with through ``numpy.random.SeedSequence``."""
        from .. import _mtgrow
        if seed is None:
            return _mtgrow.fresh_key()
        if isinstance(seed, (int, np.integer)) and 0 <= int(seed) < 2 ** 64:
            return int(seed)
        return int(np.random.SeedSequence(seed).generate_state(1, np.uint64)[0])

    def _same_tables(self, a, b, h=0):
        """ref:1819-1843 on two trees' capacity tables."""
        if a["feat"][h] < 0 or b["feat"][h] < 0:
            return bool(a["feat"][h] < 0 and b["feat"][h] < 0)
        if a["feat"][h] != b["feat"][h]:
            return False
        if a["feat"][h] < self.c_dim_continuous and not np.allclose(a["thr"][h], b["thr"][h]):
            return False
        C = int(self.c_num_children_vec[0])
        return all(self._same_tables(a, b, C * h + 1 + i) for i in range(C))

    def _forest_from_tables(self, trees, prob):
        """ref:1845-1856 and the flattening: equal trees are merged (the earlier hands its probability to the later), then
        every tree's reachable slots become breadth-first tables with the state the engine left in them."""
        trees, prob = list(trees), np.array(prob, dtype=float)
        for i in range(len(trees)):
            for j in range(i + 1, len(trees)):
                if self._same_tables(trees[i], trees[j]):
                    trees[i] = None
                    prob[j] += prob[i]
                    prob[i] = -1
                    break
        trees, prob = [t for t in trees if t is not None], prob[prob > -0.5]
        C = int(self.c_num_children_vec[0])
        tree_off, feat, child0, nchild, thr_off, depth, thr = [0], [], [], [], [], [], []
        g, post, lml, lcm = [], [], [], []
        for t in trees:
            order, base_i, i = [(0, 0)], len(feat), 0
            while i < len(order):
                h, d = order[i]
                k = int(t["feat"][h])
                feat.append(k)
                depth.append(d)
                g.append(0.0 if d == self.c_max_depth else float(t["g"][h]))
                post.append(t["post"][h])
                lml.append(0.0 if np.isnan(t["lml"][h]) and h > 0 else float(t["lml"][h]))    # (an empty child: ref:2323)
                lcm.append(float(t["lcm"][h]))
                if k < 0:
                    child0.append(0)
                    nchild.append(0)
                    thr_off.append(-1)
                else:
                    child0.append(base_i + len(order))
                    nchild.append(C)
                    if k < self.c_dim_continuous:
                        thr_off.append(len(thr))
                        thr.extend(np.asarray(t["thr"][h], dtype=float)[:C + 1])
                    else:
                        thr_off.append(-1)
                    order.extend((C * h + 1 + c, d + 1) for c in range(C))
                i += 1
            tree_off.append(len(feat))
        flat = _mtree.FlatForest(np.array(tree_off, np.int32), np.array(feat, np.int32), np.array(child0, np.int32),
                                 np.array(nchild, np.int32), np.array(thr_off, np.int32), np.array(depth, np.int32),
                                 np.array(thr, np.float64))
        _mtree.check_limits(flat.n_trees, flat.max_tree_nodes, flat.max_children, flat.max_depth, self._degree)
        state = dict(g=np.array(g, float), post=np.array(post, float).reshape(len(g), -1), lml=np.array(lml, float),
                     lcm=np.array(lcm, float), prob=prob)
        return _Forest(flat, state)

    def _mtmcmc(self, xc, xk, y, burn_in=100, num_metatrees=500, g_max=0.0, rho=0.99, phi=0.999, p_obj=0.3,
                threshold_type="1d_kmeans", seed=None):
        """ref:2029-2133: one Metropolis-Hastings chain over tree structures with an adaptive g_max during burn-in."""
        from .. import _mtgrow
        self._mcmc_checks(threshold_type)
        key = self._mcmc_key(seed)
        grower = self._grower("MTMCMC", 1, threshold_type, xc, xk, y)
        try:
            _, bad = grower.start(_mtgrow.node_table(key, 0, 1, grower.cap))
            if bad > 0:
                self._raise_bad(grower.xk)
            trees, counts = [grower.snapshot(0)], [1]
            if self.c_dim_features == 1:
                return self._forest_from_tables(trees, np.array([1.0]))
            proposed = accepted = 1
            numerator = denominator = 0.0
            trace = self._mcmc_trace = dict(out=[], g_max=[])
            g_acc = g_den = 0.0

            def step():
                nonlocal proposed, accepted, numerator, denominator
                out = grower.step(_mtgrow.node_table(key, proposed, 1, grower.cap), _mtgrow.aux_table(key, proposed, 1), None,
                                  g_max)
                trace["out"].append(out)
                numerator *= rho
                denominator = denominator * rho + 1
                if out[0, 0] > 0:
                    trees.append(grower.snapshot(0))
                    counts.append(1)
                    accepted += 1
                    numerator += 1
                else:
                    counts[-1] += 1
                proposed += 1
                print(f"\r{proposed}(accepted:{accepted})", end="")

            print(f"brun_in: {burn_in}")
            while proposed < burn_in:
                step()
                p_hat = numerator / denominator                   # _update_g_max (ref:2623-2634)
                g_new = g_max * p_obj / p_hat if p_hat > p_obj else 1.0 - (1.0 - g_max) * (1.0 - p_obj) / (1.0 - p_hat)
                g_acc = g_acc * phi + g_new
                g_den = g_den * phi + 1
                g_max = g_acc / g_den
                trace["g_max"].append(g_max)
            print()
            tmp = accepted - 1
            counts[-1] = 1
            print(f"burn_in + num_metatrees: {burn_in + num_metatrees}")
            while proposed < burn_in + num_metatrees:
                step()
            print()
            prob = np.array(counts[tmp:], dtype=float)
            return self._forest_from_tables(trees[tmp:], prob / prob.sum())
        finally:
            grower.close()

    def _remtmcmc(self, xc, xk, y, burn_in=100, num_metatrees=500, num_chains=8, g_max=0.9, beta_vec=None, num_interval=10,
                  num_exchange=4, threshold_type="1d_kmeans", seed=None):
        """ref:2135-2256: num_chains tempered chains with replica exchange; only the last chain's trees are kept."""
        from .. import _mtgrow
        self._mcmc_checks(threshold_type, num_chains)
        B = int(num_chains)
        beta = (np.arange(B) + 1) / B
        if beta_vec is not None:
            beta[:] = beta_vec
            if np.any(beta < 0) or np.any(beta > 1):
                raise ParameterFormatError(f"All the elements of beta_vec must be in [0,1] beta_vec = {beta_vec}.")
        num_interval = _check.pos_int(num_interval, "num_interval", ParameterFormatError)
        num_exchange = _check.pos_int(num_exchange, "num_exchange", ParameterFormatError)
        key = self._mcmc_key(seed)
        grower = self._grower("REMTMCMC", B, threshold_type, xc, xk, y)
        try:
            l_lasts, bad = grower.start(_mtgrow.node_table(key, 0, B, grower.cap))
            if bad > 0:
                self._raise_bad(grower.xk)
            l_lasts = np.array(l_lasts, dtype=float)
            trees, counts = [grower.snapshot(B - 1)], [1]          # the last chain's list; the others keep one tree each
            if self.c_dim_features == 1:
                return self._forest_from_tables(trees, np.array([1.0]))
            t = 0
            trace = self._mcmc_trace = dict(out=[], exchange=[])

            def step(i):
                nonlocal t
                t += 1
                aux = _mtgrow.aux_table(key, t, B, num_exchange)
                out = grower.step(_mtgrow.node_table(key, t, B, grower.cap), aux[:B], beta, g_max)
                trace["out"].append(out)
                ok = out[:, 0] > 0
                l_lasts[ok] = out[ok, 1]
                if ok[B - 1]:
                    trees.append(grower.snapshot(B - 1))
                    counts.append(1)
                else:
                    counts[-1] += 1
                if B > 1 and i % num_interval == 0:                # _replica_exchange_memory_efficient (ref:2580-2610)
                    trace["exchange"].append(-1)
                    for e in range(num_exchange):
                        j = min(B - 2, int(np.floor(aux[B + 2 * e] * (B - 1))))
                        if aux[B + 2 * e + 1] < np.exp(l_lasts[j] * beta[j + 1] + l_lasts[j + 1] * beta[j]
                                                       - l_lasts[j] * beta[j] - l_lasts[j + 1] * beta[j + 1]):
                            grower.swap(j)
                            trace["exchange"].append(j)
                            l_lasts[[j, j + 1]] = l_lasts[[j + 1, j]]
                            if j == B - 2:                         # the last chain takes chain j's tree as a new entry
                                counts[-1] -= 1
                                trees.append(grower.snapshot(B - 1))
                                counts.append(1)
                print(f"\r{i}", end="")

            print(f"brun_in: {burn_in}")
            for i in range(burn_in):
                step(i)
            print()
            tmp = len(counts) - 1
            counts[-1] = 1
            print(f"num_metatrees: {num_metatrees}")
            for i in range(num_metatrees):
                step(i)
            print()
            prob = np.array(counts[tmp:], dtype=float)
            return self._forest_from_tables(trees[tmp:], prob / prob.sum())
        finally:
            grower.close()

    def update_posterior(self, x_continuous=None, x_categorical=None, y=None, alg_type="MTRF", **kwargs):
        """ref:2667-2818 in batch form; a refused sample changes nothing."""
        xc, xk, n = self._check_sample_x(x_continuous, x_categorical)
        y = self._check_sample_y(y, xc)
        _check.shape_consistency(n, "x_continuous.shape[0] and x_categorical.shape[0]", y.shape[0], "y.shape[0]",
                                 ParameterFormatError)
        if alg_type in ("MTMCMC", "REMTMCMC"):
            if isinstance(xk, np.ndarray):
                self._check_values(xk)
            run = self._mtmcmc if alg_type == "MTMCMC" else self._remtmcmc
            self._set_hn(run(xc, xk, y, **kwargs))
            return self
        if alg_type not in ("MTRF", "given_MT"):
            return self                     # (the reference falls through its chain of elifs, ref:2806-2818)
        if alg_type == "MTRF" or isinstance(xk, np.ndarray):
            # before scikit-learn sees the sample and before the forest is replaced; a tensor handed to 'given_MT' is left
            # to the route pass, which refuses it with the state untouched
            self._check_values(xk)
        if alg_type == "MTRF":
            self._set_hn(self._mtrf(xc, xk, y, **kwargs))
        elif self._hn is None:
            raise ParameterFormatError("given_MT is supported only when len(self.hn_metatree_list) > 0.")
        eng = self._eng()
        xcd, xkd = eng.adopt_x(xc, xk)
        _, bad = eng.update(xcd, xkd, eng.adopt_y(y))
        if bad > 0:
            self._raise_bad(xkd)
        return self

    def fit(self, x_continuous=None, x_categorical=None, y=None, alg_type="MTRF", **kwargs):
        self.reset_hn_params()
        return self.update_posterior(x_continuous, x_categorical, y, alg_type, **kwargs)

    # ---- the MAP tree ------------------------------------------------------------------------------------------------------
    def _map_add_nodes(self, node):
        """ref:2820-2853: the full default subtree below a leaf that the rule lets grow."""
        if node.depth == self.c_max_depth or not node.k_candidates:
            node.h_g = 0.0
            node.sub_model = self._new_sub().set_hn_params(**self.sub_hn_params)
            node.leaf = True
            node.map_leaf = True
            return
        k = node.k = node.k_candidates[self.hn_k_weight_vec[node.k_candidates].argmax()]
        n_children = int(self.c_num_children_vec[k])
        node.thresholds = np.linspace(node.ranges[k, 0], node.ranges[k, 1], n_children + 1) if k < self.c_dim_continuous else None
        cand = _child_candidates(node.k_candidates, k, self.c_num_assignment_vec)
        node.children = []
        for i in range(n_children):
            child = _Node(node.depth + 1, cand, self.hn_g, ranges=np.array(node.ranges))
            if node.thresholds is not None:
                child.ranges[k, 0] = node.thresholds[i]
                child.ranges[k, 1] = node.thresholds[i + 1]
            node.children.append(child)
            self._map_add_nodes(child)

    def _map(self, node):
        """ref:2855-2883: the larger of stopping here and the best subtree; a leaf that can still grow is compared with
        the full default subtree below it."""
        if node.leaf:
            if node.depth == self.c_max_depth or not node.k_candidates:
                node.map_leaf = True
                return 1.0
            total, level = 0, 1
            widths = np.sort(self.c_num_children_vec[node.k_candidates])
            for i in range(min(self.c_max_depth - node.depth, len(node.k_candidates))):
                total += level
                level *= widths[i]
            grown = node.h_g * self.hn_g ** (total - 1)
            if 1.0 - node.h_g > grown:
                node.map_leaf = True
                return 1.0 - node.h_g
            self._map_add_nodes(node)
            return grown
        stay, go = 1.0 - node.h_g, node.h_g
        for child in node.children:
            go *= self._map(child)
        node.map_leaf = bool(stay > go)
        return stay if node.map_leaf else go

    def _copy_map_tree(self, out, node):
        """ref:2885-2910."""
        out.h_g = node.h_g
        if node.map_leaf:
            out.sub_model = node.sub_model
            out.leaf = True
            return
        out.k = node.k
        out.thresholds = np.array(node.thresholds) if node.k < self.c_dim_continuous else None
        cand = _child_candidates(out.k_candidates, out.k, self.c_num_assignment_vec)
        out.leaf = False
        out.children = []
        for i, child in enumerate(node.children):
            new = _Node(out.depth + 1, cand, ranges=np.array(out.ranges))
            if out.thresholds is not None:
                new.ranges[out.k, 0] = out.thresholds[i]
                new.ranges[out.k, 1] = out.thresholds[i + 1]
            out.children.append(new)
            self._copy_map_tree(new, child)

    def estimate_params(self, loss="0-1", visualize=True, filename=None, format=None):
        """The approximate MAP meta-tree (ref:2912-2992).  Plotting is out of scope: pass ``visualize=False``.  Unlike the
        reference, the ``map_leaf`` flags and the default nodes that its recursion appends are not kept in the posterior;
        the winning tree's index and flags (breadth-first) are left in ``_last_map``."""
        if loss != "0-1":
            raise CriteriaError("Unsupported loss function! This function supports only \"0-1\".")
        if visualize:
            raise NotImplementedError(_mtree.PLOT_MSG)
        map_root = _Node(0, list(self._root_k_candidates), self.hn_g, ranges=np.array(self.c_ranges), leaf=True)
        trees = self.hn_metatree_list
        if not trees:
            warnings.warn("self.hn_metatree_list is empty. Therefore, one of the most likely model tree will be returned.",
                          ResultWarning)
            self._map(map_root)
            self._last_map = (None, [])
            return map_root
        prob = self.hn_metatree_prob_vec
        best, best_p = 0, -1.0
        for i, root in enumerate(trees):
            p = prob[i] * self._map(root)
            if p > best_p:
                best, best_p = i, p
        self._copy_map_tree(map_root, trees[best])
        flags, order = [], [trees[best]]
        for node in order:
            flags.append(bool(node.map_leaf))
            if not node.leaf:
                order.extend(node.children)
        self._last_map = (best, flags)
        return map_root

    def visualize_posterior(self, filename=None, format=None, num_metatrees=3, h_params=False):
        raise NotImplementedError(_mtree.PLOT_MSG)

    # ---- prediction --------------------------------------------------------------------------------------------------------
    def get_p_params(self):
        return None

    def calc_pred_dist(self, x_continuous=None, x_categorical=None):
        """Keeps the rows; the per-node predictive values are derived from the posterior tables when a read-out asks."""
        xc, xk, n = self._check_sample_x(x_continuous, x_categorical)
        self._check_values(xk)            # (a value outside its range would silently end the walk at its node)
        self._p_x, self._p_n = (xc, xk), n
        return self

    def _predict(self, mode):
        if self._hn is None:
            raise ParameterFormatError("the prediction needs a posterior forest: len(self.hn_metatree_list) must be > 0.")
        if self._p_x is None:
            xc = np.zeros((1, self.c_dim_continuous)) if self.c_dim_continuous else None
            xk = np.zeros((1, self.c_dim_categorical), dtype=int) if self.c_dim_categorical else None
        else:
            xc, xk = self._p_x
        eng = self._eng()
        xcd, xkd = eng.adopt_x(xc, xk)
        return eng, xcd, xkd, (None if mode is None else eng.predict(xcd, xkd, mode))

    def make_prediction(self, loss=None):
        if loss is None:
            loss = "squared" if self.SubModel in REG_MODELS else "0-1"
        if loss == "squared":
            if self.SubModel not in REG_MODELS:
                raise CriteriaError("Unsupported loss function! \"squared\" is supported only when self.SubModel is normal, "
                                    "linearregression, exponential, or poisson.")
            return self._predict(_mtree.PRED_MEAN)[3]
        if loss == "0-1" or loss == "KL":
            if self.SubModel not in CLF_MODELS:
                raise CriteriaError(f"Unsupported loss function! \"{loss}\" is supported only when self.SubModel is bernoulli "
                                    "or categorical.")
            return self._predict(_mtree.PRED_CLASS if loss == "0-1" else _mtree.PRED_PROBA)[3]
        raise CriteriaError("Unsupported loss function! This function supports \"squared\", \"0-1\", and \"KL\".")

    def pred_and_update(self, x_continuous=None, x_categorical=None, y=None, loss=None):
        self.calc_pred_dist(x_continuous, x_categorical)
        prediction = self.make_prediction(loss=loss)
        self.update_posterior(x_continuous, x_categorical, y, alg_type="given_MT")
        return prediction

    def calc_pred_var(self):
        if self.SubModel not in (normal, linearregression):
            raise ParameterFormatError("SubModel must be normal or linearregression.")
        return self._predict(_mtree.PRED_VAR)[3]

    def calc_pred_density(self, y):
        """ref:3479-3529.  The node values depend on the row's y, so this is host work over the path table of
        ``mtree_route`` (not a throughput path)."""
        y = self._check_sample_y(np.asarray(y) if not hasattr(y, "shape") else y)
        y = np.asarray(y.cpu() if hasattr(y, "cpu") else y)
        try:
            y = y + np.zeros(self._p_n, dtype=y.dtype)
        except ValueError:
            raise DataFormatError(f"y must have a size that is broadcastable to ({self._p_n},). Here, {self._p_n} is the "
                                  "sample size of x when you called calc_pred_dist(x). ") from None
        eng, xcd, xkd, _ = self._predict(None)
        paths = eng.paths(xcd, xkd)
        state = eng.get_state()
        out = np.zeros(self._p_n)
        subs = {}
        if self._family == _mtree.LINREG:
            x_host = np.asarray(xcd.cpu(), dtype=float)

            def node_density(v, rows):
                """Student-t with loc x . mu_v, scale lambda_v(x)^-1/2, df 2 alpha_v (ref: linearregression :722-730)."""
                from scipy import stats
                if v not in subs:
                    subs[v] = self._lr_parts(state["post"][v])
                mu, lam, alpha, beta, _ = subs[v]
                x = x_host[rows]
                lambdas = alpha / beta / (1.0 + np.sum(x.T * np.linalg.solve(lam, x.T), axis=0))
                return stats.t.pdf(y[rows], loc=x @ mu, scale=1.0 / np.sqrt(lambdas), df=2.0 * alpha)
        else:
            def node_density(v, rows):
                if v not in subs:
                    subs[v] = self._sub_from(state["post"][v])
                return subs[v]._calc_pred_density(y[rows])
        for b in range(paths.shape[0]):
            val = np.zeros(self._p_n)
            for j in range(paths.shape[2] - 1, -1, -1):
                col = paths[b, :, j]
                for v in np.unique(col[col >= 0]):
                    rows = col == v
                    own = node_density(v, rows)
                    last = (paths[b, rows, j + 1] < 0) if j + 1 < paths.shape[2] else np.ones(rows.sum(), bool)
                    g = state["g"][v]
                    val[rows] = np.where(last, own, (1 - g) * own + g * val[rows])
            out += state["prob"][b] * val
        return out

    def calc_feature_importances(self):
        """ref:3452-3477 on the node tables."""
        forest = self._hn_forest()
        out = np.zeros(self.c_dim_features)
        if forest is None:
            return out
        fl, st = forest.flat, forest.state
        acc = np.zeros((fl.n_nodes, self.c_dim_features))
        for v in range(fl.n_nodes - 1, -1, -1):
            if fl.feat[v] < 0:
                continue
            kids = slice(int(fl.child0[v]), int(fl.child0[v]) + int(fl.nchild[v]))
            tmp = acc[kids].sum(0)
            tmp[fl.feat[v]] += st["lml"][kids].sum() - st["lml"][v]
            acc[v] = st["g"][v] * tmp
        for b in range(fl.n_trees):
            out += st["prob"][b] * acc[fl.tree_off[b]]
        return out

    def predict(self, x_continuous=None, x_categorical=None):
        self.calc_pred_dist(x_continuous, x_categorical)
        return self.make_prediction()

    def predict_proba(self, x_continuous=None, x_categorical=None):
        if self.SubModel not in CLF_MODELS:
            raise ParameterFormatError("SubModel must be bernoulli or categorical.")
        self.calc_pred_dist(x_continuous, x_categorical)
        return self.make_prediction(loss="KL")
