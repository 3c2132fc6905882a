"""The host tree logic of contexttree.LearnModel on the MI355X: the walk of tests/test_contexttree_nodes.py through a model on
the dense engine and through one on the sparse engine, at the same shapes, must give the same canonical lists bit for bit
(the two engines' updates and MAP flags are bit-equal, tests/test_gpu_contexttree_sparse.py; the host logic is one
implementation over two stores)."""
import functools

import pytest

import contexttree_sparse_oracle as sorc
from test_contexttree_nodes import LENGTHS, SHAPES, same_bits, shape_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("k,D", SHAPES)
def test_dense_and_sparse_walks_are_bit_equal(k, D, length):
    """``drive`` (updates, predictive distributions, the MAP tree, the trace, the node count), then
    ``set_hn_params(hn_root=planted_tree)``, a pickle round trip, one more ``pred_and_update`` and the MAP tree again."""
    from bayesml_amd import _ctree, _ctsp, contexttree as ct
    case = shape_case(k, D, length)
    inp = sorc.case_inputs(case)
    dense, md = sorc.extended_drive(ct, case, inp, make=functools.partial(ct.LearnModel, tables="dense", device="cuda:0"))
    sparse, ms = sorc.extended_drive(ct, case, inp, make=functools.partial(ct.LearnModel, tables="sparse", device="cuda:0"))
    assert isinstance(md._engine, _ctree.CtreePass) and isinstance(ms._engine, _ctsp.SparseCtreePass)
    assert same_bits(dense, sparse)
    assert {"after1_g", "map_leaf", "trace_p", "final_nodes", "planted_g", "unpickled_after_g", "planted_map_g"} <= set(dense)
    assert same_bits(sorc.stage_lists(dense, "planted"), sorc.stage_lists(dense, "unpickled"))
