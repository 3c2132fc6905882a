"""``contexttree.GenModel`` / ``LearnModel``: drop-in for ``bayesml/contexttree/_contexttree.py`` (cited below as
``ref:<lines>``).

The reference keeps the posterior as a tree of Python ``_Node`` objects and walks it once per symbol (ref:688-731).  Here
the posterior lives in dense per-level tables on the device (``_ctree.CtreePass``) and ``update_posterior`` is the batch
form of DESIGN.md "Context tree": ``ctree_count`` counts every (context, symbol) pair of the sample where it lies, one host
read of ``[n | bad]`` decides whether the sample is accepted, and ``ctree_sweep`` applies the update level by level.
``estimate_params`` runs ``ctree_map`` and builds only the pruned MAP tree.  ``pred_and_update_sequence`` is the per-symbol
loop of ``pred_and_update`` over a whole sample in its level-wise form (``_ctseq.SequencePass``); ``calc_pred_logpdf`` scores a
held-out sample under the posterior as it stands, every position at once (``_ctpred.PredPass``).  What touches one root-to-leaf path
(``calc_pred_dist``, ``pred_and_update``) gathers its D + 1 rows and works on the host.  ``hn_root`` is a property that
materialises the ``_Node`` tree from the tables on demand; a tree given to a setter is scattered into them.

With ``tables="sparse"`` the posterior lives in per-level hash tables that hold only the nodes that exist
(``_ctsp.SparseCtreePass``, the same update by the ``ctsp_*`` entry points).  What differs between the two storages on the
host is a store of ``_nodes``, chosen at construction; the tree algorithms are written once there, on (level, key).

``GenModel`` is host NumPy: the chain is sequential and short.
"""
from __future__ import annotations

import numpy as np

from .. import _check, _ctpred, _ctree, _ctseq, base
from . import _nodes
from .._exceptions import CriteriaError, DataFormatError, ParameterFormatError

_INT_VEC_MSG = " must be a 1-dimensional numpy.ndarray whose dtype is int. Its values must be non-negative (including 0)."


class _Node:
    """ref:16-28, attribute for attribute."""

    def __init__(self, depth, c_k, h_g=0.5):
        self.depth = depth
        self.children = [None for i in range(c_k)]  # child nodes
        self.h_g = h_g
        self.h_beta_vec = np.ones(c_k) / 2
        self.theta_vec = np.ones(c_k) / c_k
        self.leaf = False
        self.map_leaf = False


def _copy_h_tree(node, orig, c_k, c_d_max, g, beta_vec):
    """The reference's ``_set_h_params_recursion`` family (ref:175-195, 504-533): superpose ``orig`` on ``node``; where
    ``orig`` ends, the defaults ``g`` / ``beta_vec`` go to ``node`` and to everything below it."""
    if orig is None:
        node.h_g = 0.0 if node.depth == c_d_max else g
        node.h_beta_vec[:] = beta_vec
        for child in node.children:
            if child is not None:
                _copy_h_tree(child, None, c_k, c_d_max, g, beta_vec)
        return
    node.h_g = orig.h_g
    node.h_beta_vec[:] = orig.h_beta_vec
    if node.depth == c_d_max:
        node.leaf = True
        node.h_g = 0.0
    elif orig.leaf:
        node.leaf = True
    else:
        node.leaf = False
        for i in range(c_k):
            if node.children[i] is None:
                node.children[i] = _Node(node.depth + 1, c_k)
            _copy_h_tree(node.children[i], orig.children[i], c_k, c_d_max, g, beta_vec)


def _fill_tree(node, c_d_max, g=None, beta_vec=None):
    """ref:163-173: a new default for every node of an existing tree."""
    if g is not None:
        node.h_g = 0.0 if node.depth == c_d_max else g
    if beta_vec is not None:
        node.h_beta_vec[:] = beta_vec
    for child in node.children:
        if child is not None:
            _fill_tree(child, c_d_max, g, beta_vec)


class GenModel(base.Generative):
    """Data-generating model and its prior (ref:30-420; plotting is out of scope)."""

    def __init__(self, c_k, c_d_max=2, root=None, h_g=0.5, h_beta_vec=None, h_root=None, seed=None):
        self.c_k = _check.pos_int(c_k, "c_k", ParameterFormatError)
        self.c_d_max = _check.pos_int(c_d_max, "c_d_max", ParameterFormatError)
        self.rng = np.random.default_rng(seed)
        self.h_g = 0.5
        self.h_beta_vec = np.ones(self.c_k) / 2
        self.h_root = None
        self.set_h_params(h_g, h_beta_vec, h_root)
        self.root = _Node(0, self.c_k, self.h_g)
        self.root.h_beta_vec[:] = self.h_beta_vec
        self.root.leaf = True
        self.set_params(root)

    def get_constants(self):
        return {"c_k": self.c_k, "c_d_max": self.c_d_max}

    def set_h_params(self, h_g=None, h_beta_vec=None, h_root=None):
        if h_g is not None:
            self.h_g = _check.float_in_closed01(h_g, "h_g", ParameterFormatError)
            if self.h_root is not None:
                _fill_tree(self.h_root, self.c_d_max, g=self.h_g)
        if h_beta_vec is not None:
            _check.pos_floats(h_beta_vec, "h_beta_vec", ParameterFormatError)
            self.h_beta_vec[:] = h_beta_vec
            if self.h_root is not None:
                _fill_tree(self.h_root, self.c_d_max, beta_vec=self.h_beta_vec)
        if h_root is not None:
            if type(h_root) is not _Node:
                raise ParameterFormatError("h_root must be an instance of contexttree._Node")
            if self.h_root is None:
                self.h_root = _Node(0, self.c_k)
            _copy_h_tree(self.h_root, h_root, self.c_k, self.c_d_max, self.h_g, self.h_beta_vec)
        return self

    def get_h_params(self):
        return {"h_g": self.h_g, "h_beta_vec": self.h_beta_vec, "h_root": self.h_root}

    def _gen_params(self, node, h_node, tree_fix):
        """ref:101-145: the tree shape (unless ``tree_fix``) and the leaves' theta_vec, drawn top-down."""
        g = self.h_g if h_node is None else h_node.h_g
        beta_vec = self.h_beta_vec if h_node is None else h_node.h_beta_vec
        node.h_g = 0.0 if node.depth == self.c_d_max else g
        node.h_beta_vec[:] = beta_vec
        if tree_fix:
            if node.leaf:
                node.theta_vec[:] = self.rng.dirichlet(beta_vec)
            else:
                for i in range(self.c_k):
                    if node.children[i] is not None:
                        self._gen_params(node.children[i], None if h_node is None else h_node.children[i], True)
        elif node.depth == self.c_d_max or self.rng.random() > g:
            node.theta_vec[:] = self.rng.dirichlet(beta_vec)
            node.leaf = True
        else:
            node.leaf = False
            for i in range(self.c_k):
                if node.children[i] is None:
                    node.children[i] = _Node(node.depth + 1, self.c_k)
                self._gen_params(node.children[i], None if h_node is None else h_node.children[i], False)

    def gen_params(self, tree_fix=False):
        self._gen_params(self.root, self.h_root, tree_fix)
        return self

    def _set_params(self, node, orig):
        """ref:147-161."""
        node.h_g = orig.h_g
        node.h_beta_vec[:] = orig.h_beta_vec
        node.theta_vec[:] = orig.theta_vec
        if node.depth == self.c_d_max:
            node.leaf = True
            node.h_g = 0.0
        elif orig.leaf:
            node.leaf = True
        else:
            node.leaf = False
            for i in range(self.c_k):
                if node.children[i] is None:
                    node.children[i] = _Node(node.depth + 1, self.c_k)
                self._set_params(node.children[i], orig.children[i])

    def set_params(self, root=None):
        if root is not None:
            if type(root) is not _Node:
                raise ParameterFormatError("root must be an instance of contexttree._Node")
            self._set_params(self.root, root)
        return self

    def get_params(self):
        return {"root": self.root}

    def gen_sample(self, sample_length, initial_values=None):
        """ref:323-355: the chain starts from ``initial_values`` (zeros by default), which are not returned."""
        _check.pos_int(sample_length, "sample_length", DataFormatError)
        x = np.zeros(sample_length + self.c_d_max, dtype=int)
        if initial_values is not None:
            _check.nonneg_ints(initial_values, "initial_values", DataFormatError)
            _check.shape_consistency(initial_values.shape[0], "initial_values.shape[0]", self.c_d_max, "self.c_d_max",
                                     DataFormatError)
            if initial_values.max() >= self.c_k:
                raise DataFormatError(f"initial_values.max() must smaller than c_k:{self.c_k}")
            x[:self.c_d_max] = initial_values
        for i in range(self.c_d_max, sample_length + self.c_d_max):
            node = self.root
            while not node.leaf:
                node = node.children[x[i - node.depth - 1]]
            x[i] = self.rng.choice(self.c_k, p=node.theta_vec)
        return x[self.c_d_max:]

    def save_sample(self, filename, sample_length, initial_values=None):
        np.savez_compressed(filename, self.gen_sample(sample_length, initial_values))

    def visualize_model(self, filename=None, format=None, sample_length=10):
        _check.pos_int(sample_length, "sample_length", DataFormatError)
        raise NotImplementedError(_ctree.PLOT_MSG)


class LearnModel(base.Posterior, base.PredictiveMixin):
    """Posterior and predictive distribution (ref:422-1067).  Positional parameters are the reference's; keyword-only
    ``device`` selects the GPU.  The dense tables limit the shape to ``c_k <= 256`` and ``c_k ** (c_d_max + 1) <= 2 ** 24``
    (``EngineLimitError`` beyond; the reference has no such limit).  Keyword-only ``tables="sparse"`` stores only the nodes
    that exist, in per-level hash tables on the device (``_ctsp.SparseCtreePass``): the limit is then
    ``ceil(log2 c_k) * c_d_max <= 63`` and the memory the nodes take.  ``tables="dense"`` is the default.

    The engine, and with it the GPU, is first needed when a posterior tree exists: at the first ``update_posterior`` or
    ``pred_and_update`` - or already in the constructor (and in ``set_h0_params`` / ``set_hn_params``) when a tree is given
    as ``h0_root`` / ``hn_root``, because it is scattered into the device tables at once.  Without a GPU those calls raise
    ``EngineUnavailableError``; a model without a tree is built on the host alone."""

    _ctree_pass_factory = None        # private test seam (tests/fake_contexttree_engine.py)
    _ctseq_pass_factory = None        # private test seam (tests/contexttree_seq_oracle.py)
    _ctpred_pass_factory = None       # private test seam (tests/contexttree_pred_oracle.py)
    _seq_pass = None
    _pred_pass = None
    _sparse = False                   # (a model pickled before the keyword existed is dense)

    def __init__(self, c_k, c_d_max=2, h0_g=0.5, h0_beta_vec=None, h0_root=None, *, tables="dense", device=None):
        self.c_k = _check.pos_int(c_k, "c_k", ParameterFormatError)
        self.c_d_max = _check.pos_int(c_d_max, "c_d_max", ParameterFormatError)
        if tables not in ("dense", "sparse"):
            raise ParameterFormatError("tables must be \"dense\" or \"sparse\"")
        self._sparse = tables == "sparse"
        self._store = _nodes.store_for(self._sparse, self.c_k, self.c_d_max)
        self._device = device
        self._engine = None
        self._saved_tables = None
        self._has_root = False
        self._off = self._store.off

        self.h0_g = h0_g
        self.h0_beta_vec = np.ones(self.c_k) / 2
        self.h0_root = None
        self.hn_g = h0_g
        self.hn_beta_vec = np.ones(self.c_k) / 2
        self.p_theta_vec = np.ones(self.c_k) / self.c_k
        self.set_h0_params(h0_g, h0_beta_vec, h0_root)

    # ---- the engine and its tables ---------------------------------------------------------------------------------------
    def _eng(self):
        if self._engine is None:
            self._engine = self._store.make_engine(self)
            if self._saved_tables is not None:
                self._store.restore(self._engine, self._saved_tables)
                self._saved_tables = None
        return self._engine

    def __getstate__(self):
        state = dict(self.__dict__)
        if self._engine is not None and self._has_root:
            state["_saved_tables"] = self._store.save(self._engine)
        state["_engine"] = None
        state.pop("_seq_pass", None)
        state.pop("_pred_pass", None)
        state.pop("_store", None)           # (derived on loading: the state keeps the layout it always had)
        return state

    def __getattr__(self, name):
        if name != "_store":
            raise AttributeError(name)
        self._store = _nodes.store_for(self._sparse, self.c_k, self.c_d_max)      # (a model restored from a pickled state)
        return self._store

    def get_constants(self):
        return {"c_k": self.c_k, "c_d_max": self.c_d_max}

    def _default_g(self, depth):
        return 0.0 if depth == self.c_d_max else self.hn_g

    @property
    def hn_root(self):
        """The posterior as the reference's ``_Node`` tree (a fresh copy: host work proportional to the existing nodes),
        or ``None`` before the first update."""
        if not self._has_root:
            return None
        return _nodes.hn_root(self, _Node)

    # ---- hyperparameters ---------------------------------------------------------------------------------------------------
    def set_h0_params(self, h0_g=None, h0_beta_vec=None, h0_root=None):
        if h0_g is not None:
            self.h0_g = _check.float_in_closed01(h0_g, "h0_g", ParameterFormatError)
            if self.h0_root is not None:
                _fill_tree(self.h0_root, self.c_d_max, g=self.h0_g)
        if h0_beta_vec is not None:
            _check.pos_floats(h0_beta_vec, "h0_beta_vec", ParameterFormatError)
            self.h0_beta_vec[:] = h0_beta_vec
            if self.h0_root is not None:
                _fill_tree(self.h0_root, self.c_d_max, beta_vec=self.h0_beta_vec)
        if h0_root is not None:
            if type(h0_root) is not _Node:
                raise ParameterFormatError("h0_root must be an instance of contexttree._Node")
            if self.h0_root is None:
                self.h0_root = _Node(0, self.c_k)
            _copy_h_tree(self.h0_root, h0_root, self.c_k, self.c_d_max, self.h0_g, self.h0_beta_vec)
        self.reset_hn_params()
        return self

    def get_h0_params(self):
        return {"h0_g": self.h0_g, "h0_beta_vec": self.h0_beta_vec, "h0_root": self.h0_root}

    def set_hn_params(self, hn_g=None, hn_beta_vec=None, hn_root=None):
        if hn_g is not None:
            self.hn_g = _check.float_in_closed01(hn_g, "hn_g", ParameterFormatError)
            if self._has_root:
                self._eng().fill_existing(g=self.hn_g)
        if hn_beta_vec is not None:
            _check.pos_floats(hn_beta_vec, "hn_beta_vec", ParameterFormatError)
            self.hn_beta_vec[:] = hn_beta_vec
            if self._has_root:
                self._eng().fill_existing(beta=self.hn_beta_vec)
        if hn_root is not None:
            if type(hn_root) is not _Node:
                raise ParameterFormatError("hn_root must be an instance of contexttree._Node")
            _nodes.set_hn_root(self, hn_root)
        self.calc_pred_dist(np.zeros(self.c_d_max, dtype=int))
        return self

    def get_hn_params(self):
        return {"hn_g": self.hn_g, "hn_beta_vec": self.hn_beta_vec, "hn_root": self.hn_root}

    # ---- learning ----------------------------------------------------------------------------------------------------------
    @staticmethod
    def _check_sample(x):
        """The host half of ``_adopt_sample``: the sample as an array or tensor of a kind the engine adopts."""
        if _check._is_int(x) and x >= 0:
            x = np.asarray([x])
        if _check.sample_kind(x) != "i":
            raise DataFormatError("x" + _check.SAMPLE_MSG["nonneg_ints"])
        if (x.numel() if hasattr(x, "numel") else x.size) == 0:
            np.max(np.zeros(0))          # the reference's x.max() of an empty sample: ValueError
        return x

    def _adopt_sample(self, x):
        """What ``update_posterior``, ``pred_and_update_sequence`` and ``calc_pred_logpdf`` accept as a sample, on the
        engine's device."""
        return self._eng().adopt(self._check_sample(x))

    def _refuse_bad_symbols(self, xd, bad):
        """``bad`` symbols were counted outside 0..c_k-1: the reference's message for a negative one, else for a large one."""
        if bad > 0:
            if self._eng().any_negative(xd):
                raise DataFormatError("x" + _check.SAMPLE_MSG["nonneg_ints"])
            raise DataFormatError(f"x.max() must smaller than c_k:{self.c_k}")

    def _ensure_root(self):
        """A model without a tree gets its root, with the defaults, before a path or the MAP sweep starts from it."""
        if not self._has_root:
            eng = self._eng()
            eng.clear()
            eng.scatter([self._store.address(0, 0)], [self.hn_g], [self.hn_beta_vec], [1], [0])
            self._has_root = True

    def update_posterior(self, x):
        """ref:712-731 in batch form; a refused sample changes nothing."""
        xd = self._adopt_sample(x)
        eng = self._eng()
        if not self._has_root:
            eng.clear()
        n, bad = eng.update(xd, self.hn_g, self.hn_beta_vec)
        self._refuse_bad_symbols(xd, bad)
        self._has_root = True
        return self

    def estimate_params(self, loss="0-1", visualize=True, filename=None, format=None):
        """The MAP tree (ref:733-831) from the engine's ``map_leaf`` flags; only the pruned tree is built.  Plotting is out
        of scope: pass ``visualize=False``.  Unlike the reference, the default-valued nodes that its sweep appends to
        ``hn_root`` are not added to the posterior."""
        if loss != "0-1":
            raise CriteriaError("Unsupported loss function! This function supports only \"0-1\".")
        if visualize:
            raise NotImplementedError(_ctree.PLOT_MSG)
        self._ensure_root()
        return _nodes.map_tree(self, _Node)

    def visualize_posterior(self, filename=None, format=None, h_params=False):
        raise NotImplementedError(_ctree.PLOT_MSG)

    # ---- prediction --------------------------------------------------------------------------------------------------------
    def get_p_params(self):
        return {"p_theta_vec": self.p_theta_vec}

    def _check_context(self, x):
        if not (_check._arr_kind(x) == "i" and x.ndim == 1 and np.all(x >= 0)):
            raise DataFormatError("x" + _INT_VEC_MSG)
        if x.max() >= self.c_k:
            raise DataFormatError(f"x.max() must smaller than c_k:{self.c_k}")

    def calc_pred_dist(self, x):
        """ref:954-989: the mixture over the path of the context x[:-1] (x[-1] is the position to predict)."""
        self._check_context(x)
        if not self._has_root:
            self.p_theta_vec[:] = self.hn_beta_vec / self.hn_beta_vec.sum()
            return self
        idx, g, beta, leaf = _nodes.path(self, x)
        p = beta[-1] / beta[-1].sum()
        for d in range(len(idx) - 2, -1, -1):
            p = (1 - g[d]) * beta[d] / beta[d].sum() + g[d] * p
        self.p_theta_vec[:] = p
        self._eng().scatter(idx, g, beta, np.ones(len(idx), np.uint8), leaf)
        return self

    @staticmethod
    def _sequence_offsets(lengths, n):
        """``lengths`` as the S + 1 starts of the sequences of a sample of n symbols (host int64), checked on the host."""
        msg = ("lengths must be a 1-dimensional array, tensor or list of non-negative integers whose sum is the length "
               "of x")
        if hasattr(lengths, "detach"):
            lengths = lengths.detach().cpu().numpy()
        try:
            arr = np.asarray(lengths)
        except Exception:
            raise DataFormatError(msg) from None
        if isinstance(lengths, (list, tuple)) and arr.size == 0:
            arr = arr.astype(np.int64)
        if arr.ndim != 1 or arr.dtype.kind not in "iu" or (arr.size and int(arr.min()) < 0):
            raise DataFormatError(msg)
        off = np.concatenate([[0], np.cumsum(arr.astype(np.int64))]).astype(np.int64)
        if int(off[-1]) != n:
            raise DataFormatError(msg)
        return off

    def calc_pred_logpdf(self, x, *, lengths=None, assign=False, return_dist=False, totals=False):
        """``ln p(x[i] | x[i-1], ..., x[i-min(i, c_d_max)], data)`` of every position of a held-out sample under the
        posterior as it stands, float64 ``[n]``, in one device pass (``_ctpred.PredPass``, DESIGN.md "Predictive
        log-probability of held-out sequences"): the logarithm of entry ``x[i]`` of what ``calc_pred_dist(x[:i + 1])``
        leaves in ``p_theta_vec`` (ref:954-989).  ``-lnp.sum()`` is the code length of the sample in nats.

        ``x`` is accepted and refused as ``update_posterior`` does it.  ``lengths`` (1-D non-negative integers summing to
        ``n``) makes ``x`` the concatenation of independent sequences: no context reaches before the start of its own
        sequence.  ``assign=True`` adds ``z``, int64 ``[n]``, the first maximum of each position's predictive vector
        (``make_prediction(loss="0-1")``); ``return_dist=True`` adds the vectors, float64 ``[n, c_k]``; ``totals=True``
        (needs ``lengths``) adds the sum of ``lnp`` over each sequence, float64 ``[S]``, 0.0 for an empty one, by a
        fixed-tree reduction that gives the same bits on every run.  With flags the return is the tuple
        ``(lnp, z, dist, totals)`` without the parts not asked for: NumPy arrays for a NumPy ``x``, tensors on the model's
        device otherwise.

        Nothing is learnt and nothing changes: unlike the reference's ``calc_pred_dist``, no default-valued node is
        appended to the tree (such a node predicts exactly what its absence predicts), and ``hn_*``, ``p_theta_vec`` and
        the tables stay as they were.  Dense and sparse tables of the same tree give the same bits.  No CPU fallback."""
        if totals and lengths is None:
            raise ParameterFormatError("totals=True sums over the sequences that lengths describes: pass lengths with it.")
        x = self._check_sample(x)
        as_numpy = not hasattr(x, "numel")
        seq_off = None
        if lengths is not None:
            seq_off = self._sequence_offsets(lengths, int(x.numel() if hasattr(x, "numel") else x.size))
        eng = self._eng()
        xd = eng.adopt(x)
        if self._pred_pass is None:
            make = self._ctpred_pass_factory
            self._pred_pass = make(eng, self._store) if make is not None else _ctpred.PredPass(eng, self._store)
        bad, lnp, z, dist, tot = self._pred_pass.run(xd, seq_off, self._has_root, self.hn_g, self.hn_beta_vec,
                                                     assign=bool(assign), dist=bool(return_dist), totals=bool(totals))
        self._refuse_bad_symbols(xd, bad)
        out = [v for v in (lnp, z, dist, tot) if v is not None]
        if as_numpy:
            out = [v.cpu().numpy() for v in out]
        return out[0] if len(out) == 1 else tuple(out)

    def make_prediction(self, loss="KL"):
        if loss == "KL":
            return self.p_theta_vec
        if loss == "0-1":
            return np.argmax(self.p_theta_vec)
        raise CriteriaError("Unsupported loss function! This function supports \"0-1\" and \"KL\".")

    def pred_and_update(self, x, loss="KL"):
        """ref:1016-1067: predict x[-1] from the context before it, then fold it in; one path, host work."""
        self._check_context(x)
        self._ensure_root()
        idx, g, beta, leaf = _nodes.path(self, x)
        a = int(x[-1])
        p = beta[-1] / beta[-1].sum()
        beta[-1, a] += 1
        for d in range(len(idx) - 2, -1, -1):
            own = beta[d] / beta[d].sum()
            beta[d, a] += 1
            mixed = (1 - g[d]) * own + g[d] * p
            g[d] = g[d] * p[a] / mixed[a]
            p = mixed
        self.p_theta_vec[:] = p
        self._eng().scatter(idx, g, beta, np.ones(len(idx), np.uint8), leaf)
        return self.make_prediction(loss=loss)

    def pred_and_update_sequence(self, x, loss="KL", *, code_length=False, chunk_bytes=None):
        """``[pred_and_update(x[:i + 1], loss) for i in range(n)]`` in one device pass per level (``_ctseq.SequencePass``,
        DESIGN.md "Sequential prediction"); the posterior is left as that loop leaves it.

        ``x`` is accepted and refused as ``update_posterior`` does it; a refused sample changes nothing.  The return is
        float64 ``[n, c_k]`` for ``loss="KL"`` and int64 ``[n]`` (the first maximum) for ``"0-1"``: NumPy arrays for a
        NumPy ``x``, tensors on the model's device for a device tensor.  With ``code_length=True`` it is
        ``(prediction, nats)``, ``nats[i] = -ln p(x[i] | x[:i])`` float64 ``[n]``.  ``loss=None`` needs
        ``code_length=True`` and returns ``nats`` alone; no ``[n, c_k]`` buffer exists then and ``p_theta_vec`` is left
        untouched (otherwise it becomes the last row).  ``chunk_bytes`` bounds the workspace (default 256 MiB): positions
        are processed in chunks of ``_ctseq.plan_chunks(...)`` positions, in order, with the state carried by the tables,
        so one call equals successive calls on the same pieces bit for bit.  Within a chunk a node's log-odds are
        carried in binary64 and stored as ``h_g`` at the chunk's end; an ``h_g`` that rounds to exactly 0 or 1 there stays,
        as it does between two calls of the reference.  Dense tables only."""
        if self._sparse:
            raise NotImplementedError("pred_and_update_sequence does not support tables=\"sparse\" in this version; "
                                      "build the model with tables=\"dense\"")
        if loss is None:
            if not code_length:
                raise CriteriaError("loss=None returns the code lengths alone: pass code_length=True with it.")
        elif not (isinstance(loss, str) and loss in ("KL", "0-1")):
            raise CriteriaError("Unsupported loss function! This function supports \"0-1\" and \"KL\".")
        xd = self._adopt_sample(x)
        as_numpy = not hasattr(x, "numel")          # (an int or a NumPy array: what is left once a tensor is ruled out)
        eng = self._eng()
        n, bad = (int(v) for v in eng.count(xd)[:2].cpu())
        self._refuse_bad_symbols(xd, bad)
        if self._seq_pass is None:
            make = self._ctseq_pass_factory
            self._seq_pass = make(eng) if make is not None else _ctseq.SequencePass(eng)
        if not self._has_root:
            eng.clear()
        want = {"KL": "rows", "0-1": "argmax", None: None}[loss]
        pred, nats, last = self._seq_pass.run(xd, self.hn_g, self.hn_beta_vec, want, bool(code_length), chunk_bytes)
        self._has_root = True
        if last is not None:
            self.p_theta_vec[:] = last.cpu().numpy()
        if as_numpy:
            pred = None if pred is None else pred.cpu().numpy()
            nats = None if nats is None else nats.cpu().numpy()
        if loss is None:
            return nats
        return (pred, nats) if code_length else pred
