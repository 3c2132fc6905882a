"""The host tree logic of contexttree.LearnModel (``contexttree/_nodes.py``) without a GPU: one implementation over the dense
and the sparse store, so the same walk through a model on the dense stand-in and on the dict-backed sparse stand-in
(tests/fake_contexttree_engine.py) must give the same canonical lists bit for bit; states pickled in the layout of earlier
versions; and c_k = 1 with an absent child."""
import pickle

import numpy as np
import pytest

import contexttree_sparse_oracle as sorc
import fake_contexttree_engine as fake
from bayesml_amd import contexttree as ct
from conftest import GOLDEN

# the smallest shapes at which key arithmetic can go wrong: k = 1 (the geometric-sum limit), D = 1, k = 3 and 5 (sparse
# symbol bits are not log2 k, so dense and sparse keys differ in form), (4, 4), (16, 2); samples of 1, D, D + 1 and 200
SHAPES = ((1, 2), (2, 1), (2, 3), (3, 2), (5, 2), (4, 4), (16, 2))
LENGTHS = ("1", "D", "D+1", "200")


class DenseModel(ct.LearnModel):
    _ctree_pass_factory = staticmethod(fake.CpuCtreePass)


class SparseModel(ct.LearnModel):
    _ctree_pass_factory = staticmethod(fake.CpuSparseCtreePass)

    def __init__(self, *a, **kw):
        super().__init__(*a, tables="sparse", **kw)


def shape_case(k, D, length):
    n = {"1": 1, "D": D, "D+1": D + 1, "200": 200}[length]
    # (the 200-symbol sample is learnt in two updates; the short ones leave nothing for a second)
    return sorc._case(f"k{k}_d{D}_n{n}", k, D, n if n < 200 else 140, 0 if n < 200 else 60, h0_g=0.4, seed=100 * k + D)


def same_bits(a, b):
    """Two dicts of arrays: the same names, shapes, dtypes and bytes (NaN rows of theta included)."""
    assert set(a) == set(b)
    for name in a:
        x, y = np.asarray(a[name]), np.asarray(b[name])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), name
    return True


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("k,D", SHAPES)
def test_dense_and_sparse_walks_are_bit_equal(k, D, length):
    """``drive`` (two updates, three predictive distributions, the MAP tree, the 50-step trace, the final node count) and
    its extension by ``set_hn_params(hn_root=...)`` and a pickle round trip."""
    case = shape_case(k, D, length)
    inp = sorc.case_inputs(case)
    dense, md = sorc.extended_drive(ct, case, inp, make=DenseModel)
    sparse, ms = sorc.extended_drive(ct, case, inp, make=SparseModel)
    assert not md._sparse and ms._sparse and isinstance(ms._engine, fake.CpuSparseCtreePass)
    assert same_bits(dense, sparse)
    assert {"after1_g", "map_leaf", "trace_p", "final_nodes", "planted_g", "unpickled_after_g", "planted_map_g"} <= set(dense)
    assert ("after2_g" in dense) == (length == "200")
    # the planted tree is in the posterior as given: the chain's values, 0 at the maximal depth, the flipped leaf
    planted = sorc.lists_to_nodes(sorc.stage_lists(dense, "planted"), k, D)
    for d in range(D + 1):
        g, beta, leaf = planted[(d, 0)]
        assert g == (0.0 if d == D else 0.15 + 0.05 * d) and leaf == (d == D)
        assert np.array_equal(beta, np.arange(1, k + 1) + d / 4.0)
    if k > 1 and D > 1:
        g, beta, leaf = planted[(1, sorc.pack([k - 1], k, D))]
        assert (g, leaf) == (0.35, 1) and np.all(beta == 3.0)
    if k > 2 and D > 1:
        # and where the tree ended (the root's middle children), whatever exists below carries the defaults again
        below = [(d, v) for (d, s), v in planted.items() if d >= 1 and sorc.unpack(s, d, k, D)[0] not in (0, k - 1)]
        assert len(below) >= k - 2
        assert all(v[0] == (0.0 if d == D else 0.4) and np.array_equal(v[1], np.arange(1, k + 1) / 2.0) for d, v in below)


def hand_made_state(sparse):
    """The state of a (2, 2) model after some learning, in the layout that ``__getstate__`` has always written: built from
    arrays here, not by the code under test.  Nodes: the root, context (1) and context (1, 0)."""
    k, D = 2, 2
    g, beta, leaf = [0.25, 0.625, 0.0], [[1.5, 3.0], [0.5, 2.0], [4.5, 1.0]], [0, 0, 1]
    if sparse:
        saved = dict(level=np.array([0, 1, 2], np.int32), key=np.array([0, 0b10, 0b10], np.int64), g=np.array(g),
                     beta=np.array(beta), leaf=np.array(leaf, np.uint8))
    else:
        at = [0, 1 + 1, 3 + 1]                            # off = [0, 1, 3, 7]; keys 1 and 1 + 0 * 2
        saved = dict(g=np.zeros(7), beta=np.zeros((7, 2)), exists=np.zeros(7, np.uint8), leaf=np.zeros(7, np.uint8))
        saved["g"][at], saved["beta"][at], saved["exists"][at], saved["leaf"][at] = g, beta, 1, leaf
    state = dict(c_k=k, c_d_max=D, _sparse=sparse, _device=None, _engine=None, _saved_tables=saved, _has_root=True,
                 _off=None if sparse else [0, 1, 3, 7], h0_g=0.5, h0_beta_vec=np.ones(2) / 2, h0_root=None, hn_g=0.5,
                 hn_beta_vec=np.ones(2) / 2, p_theta_vec=np.ones(2) / 2)
    want = dict(level=np.array([0, 1, 2], np.int32), ctx=np.array([[0, 0], [1, 0], [1, 0]], np.uint8), g=np.array(g),
                beta=np.array(beta), leaf=np.array(leaf, np.uint8))
    return state, want


@pytest.mark.parametrize("sparse", [False, True])
def test_a_state_in_the_old_layout_restores(sparse):
    state, want = hand_made_state(sparse)
    cls = SparseModel if sparse else DenseModel
    m = cls.__new__(cls)
    m.__dict__.update(pickle.loads(pickle.dumps(state)))          # what pickle does with the state of such a class
    assert same_bits(sorc.tree_to_lists(m.hn_root, 2, 2), want) and m._saved_tables is None
    # the layout is still the one written: the same keys, the tables under _saved_tables as get_tables / get_nodes give them
    again = m.__getstate__()
    assert set(again) == set(state) and again["_engine"] is None and again["_off"] == state["_off"]
    assert same_bits(again["_saved_tables"], state["_saved_tables"])
    # and the model works on: one more update, against the oracle on the hand-made nodes
    x = np.array([1, 0, 1, 1, 0, 1])
    nodes = sorc.batch_update(x, 2, 2, sorc.lists_to_nodes(want, 2, 2), 0.5, np.ones(2) / 2)
    assert same_bits(sorc.tree_to_lists(m.update_posterior(x).hn_root, 2, 2), sorc.nodes_to_lists(nodes, 2, 2))
    assert m.estimate_params(visualize=False).depth == 0


# ---- c_k = 1 with an absent child --------------------------------------------------------------------------------------------
def _k1_fixture():
    import json
    import os
    with open(os.path.join(GOLDEN, "contexttree_k1_absent_child.json")) as f:
        return json.load(f)


# What estimate_params gives where the reference has no answer (below): level, leaf and h_g of the MAP tree, every
# theta_vec = (b - 1) / (b - 1) = 1.  With c_k = 1 the full subtree below a node at depth d is a chain of D - d nodes, the
# geometric sum's limit; a node at depth D - 1 prices its missing child at hn_g ** 0 = 1.
#   k1_d2, k1_d3: h_g = 0.9 at the root, 0.7 below.  Depth D - 1: stop = 0.3 < 0.7 * max(0.3, 0.7): not a leaf, value 0.49;
#     (D = 3) depth 1: 0.3 < 0.7 * 0.49; the root: 0.1 < 0.9 * 0.49 (0.9 * 0.343).  The missing node at depth D is a leaf;
#     its parent's rule (0.3 > 0.7) does not hold, so its h_g is 0.
#   k1_d2_stops_above: depth 1 has h_g = 0.3: stop = 0.7 > 0.3 * 0.7, a leaf; the root: 0.1 < 0.9 * 0.7.
#   k1_d2_one_symbol: the root alone, h_g = 0.9 w / (0.1 + 0.9 w) with w = 1 the only symbol's probability both ways: 0.9;
#     stop = 0.1, its missing child prices at max(0.1, 0.9 * 0.9): 0.1 < 0.9 * 0.81, not a leaf, and the rule
#     (0.1 > 0.81) does not hold: the full chain below, hn_g above the maximal depth and 0 there.
K1_LIMIT_TREES = {
    "k1_d2": ([0, 1, 2], [0, 0, 1], [0.9, 0.7, 0.0]),
    "k1_d3": ([0, 1, 2, 3], [0, 0, 0, 1], [0.9, 0.7, 0.7, 0.0]),
    "k1_d2_stops_above": ([0, 1], [0, 1], [0.9, 0.3]),
    "k1_d2_one_symbol": ([0, 1, 2], [0, 0, 1], [0.9, 0.9, 0.0]),
}


@pytest.mark.parametrize("make", [DenseModel, SparseModel])
@pytest.mark.parametrize("name", [c["name"] for c in sorc.K1_CASES])
def test_k1_with_an_absent_child(name, make):
    """A missing child under an existing parent at c_k = 1.  The posterior is the reference's, value for value.  For
    ``estimate_params`` the reference has no tree to compare with: its rule (ref:757) divides by c_k - 1 and every case
    here ends in ``ZeroDivisionError: division by zero``, which the fixture records.  The drop-in defines c_k = 1 by the limit
    of the geometric sum, as its kernels always have (include/ctree.h), and returns the tree derived above
    ``K1_LIMIT_TREES``; both stores must give it."""
    case, fx = next(c for c in sorc.K1_CASES if c["name"] == name), _k1_fixture()[name]
    assert fx["map_outcome"] == ["ZeroDivisionError", "division by zero"] and fx["map"] == {}
    got = sorc.k1_drive(ct, case, make=make)
    assert got["posterior"] == fx["posterior"]
    level, leaf, g = K1_LIMIT_TREES[name]
    assert got["map_outcome"] is None
    assert (got["map"]["level"], got["map"]["leaf"], got["map"]["g"]) == (level, leaf, g)
    assert got["map"]["ctx"] == [[0] * case["D"]] * len(level) and got["map"]["theta"] == [[1.0]] * len(level)
