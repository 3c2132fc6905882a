"""``mtpred`` without a GPU: the C ABI of include/mtpred.h (header, library and ctypes table agree; argument errors come back
before the device is touched) and the refusals of ``metatree.LearnModel.calc_pred_logpdf``.
"""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import ROOT


def test_header_library_and_ctypes_table_agree():
    from bayesml_amd import _mtpred, _mtree
    text = re.sub(r"/\*.*?\*/", "", open(ROOT + "/include/mtpred.h").read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mtpred_[a-z0-9_]+)\s*\(", text)))
    lib = _mtpred.load_library()
    assert sorted(_mtpred.SYMBOLS) == declared and len(declared) == 5
    assert all(getattr(lib, name) is not None for name in declared)
    assert lib.mtpred_abi_version() == 1 == int(re.search(r"#define MTPRED_ABI_VERSION (\d+)", text).group(1))
    for macro, value in (("TILE", _mtpred.TILE), ("WAVES", _mtpred.WAVES), ("LDS_BYTES", _mtpred.LDS_BYTES), ("SHARE", _mtpred.SHARE),
                         ("LR_CONSTS", _mtpred.LR_CONSTS)):
        assert int(re.search(rf"#define MTPRED_{macro} (\d+)", text).group(1)) == value
    assert [lib.mtpred_consts_len(10, f, 3) for f in range(6)] == [20, 30, 30, 30, 40, 2600]
    assert [lib.mtpred_consts_len(*a) for a in ((0, 0, 0), (5, 6, 1), (5, 1, 0), (5, 1, 17), (5, 5, 16))] == [-1] * 5
    assert [lib.mtpred_work_len(n, t) for n, t in ((1, 1), (64, 1), (65, 1), (65, 0), (0, 1))] == [1, 1, 2, 0, -1]
    assert _mtree.load_library().mtree_abi_version() == 2


def test_argument_errors_without_a_gpu():
    from bayesml_amd import _mtpred, _mtree
    lib = _mtpred.load_library()
    P, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)                       # never dereferenced

    def call(forest=None, fam=4, deg=0, xct=4, xc=P, xkt=1, xk=P, y=P, n=10, post=P, g=P, prob=P, consts=P, lnp=P, total=None, work=None,
             **sizes):
        f = dict(n_trees=2, n_nodes=6, n_thr=3, max_tree_nodes=3, max_children=2, max_depth=1, dim_cont=2, dim_cat=1)
        f.update(sizes)
        st = _mtree.ForestStruct(*f.values(), *([4096] * 7))
        for name, ptr in (forest or {}).items():
            setattr(st, name, ptr)
        return lib.mtpred_logpdf(ctypes.byref(st), fam, deg, xct, xc, xkt, xk, y, n, post, g, prob, consts, lnp, total, work, None)

    def refused(rc, text, code=1):
        assert rc == code and text in lib.mtpred_last_error().decode(), (rc, lib.mtpred_last_error())

    assert lib.mtpred_logpdf(None, 4, 0, 4, P, 1, P, P, 10, P, P, P, P, P, None, None, None) == 1
    refused(call(n_trees=0), "inconsistent forest sizes")
    refused(call(n_trees=1025, n_nodes=2000), "not supported", code=2)
    refused(call(max_depth=25), "not supported", code=2)
    refused(call(forest={"feat_dev": None}), "null forest table")
    refused(call(forest={"thr_dev": 4100}), "misaligned forest table")
    refused(call(fam=6), "unknown family")
    refused(call(fam=1, deg=0), "degree < 1")
    refused(call(fam=1, deg=17), "not supported", code=2)
    refused(call(fam=5, deg=16), "not supported", code=2)
    refused(call(fam=5, deg=3), "must equal dim_cont")
    refused(call(n=0), "n must be >= 1")
    refused(call(n=2 ** 31 * 64), "too large")
    refused(call(xct=2), "xc_dtype")
    refused(call(xkt=3), "xk_dtype")
    for null in ("xc", "xk", "y", "post", "g", "prob", "consts", "lnp"):
        refused(call(**{null: None}), "null pointer")
    refused(call(total=P), "null pointer")                                      # a total needs work_dev
    refused(call(xc=odd), "xc_dev must be aligned")
    refused(call(xk=ctypes.c_void_p(4098)), "xk_dev must be aligned")
    for name in ("y", "post", "g", "prob", "consts", "lnp"):
        refused(call(**{name: odd}), "8-byte aligned")


def _model(forest=True):
    from bayesml_amd import metatree, poisson
    leaf = lambda: metatree._Node(1, sub_model=poisson.LearnModel(), leaf=True)          # noqa: E731
    root = metatree._Node(0, k=1, sub_model=poisson.LearnModel(), children=[leaf(), leaf()])
    return metatree.LearnModel(1, 1, c_max_depth=1, SubModel=poisson, **({"h0_metatree_list": [root]} if forest else {}))


def test_the_method_refuses_as_its_neighbours_do():
    from bayesml_amd._engine import EngineUnavailableError
    from bayesml_amd._exceptions import DataFormatError, ParameterFormatError
    x, k, y = np.zeros((4, 1)), np.array([[0], [1], [0], [1]]), np.array([0, 3, 1, 2])
    with pytest.raises(ParameterFormatError, match="needs a posterior forest"):
        _model(forest=False).calc_pred_logpdf(x, k, y)
    m = _model().calc_pred_dist(x[:2], k[:2])
    kept = m._p_x
    for args, err in (((x, k, y.astype(float)), DataFormatError), ((x, k, y[:3]), ParameterFormatError), ((x, k, -y), DataFormatError),
                      ((x, k, None), DataFormatError), ((x, k + 1, y), DataFormatError), ((x, -k, y), DataFormatError),
                      ((x[:, :0], k, y), ParameterFormatError), ((x, k.astype(float), y), DataFormatError)):
        with pytest.raises(err):
            m.calc_pred_logpdf(*args)
        assert m._p_x is kept and m._p_n == 2 and m._engine is None
    assert m.calc_pred_logpdf.__kwdefaults__ == {"total": False}
    for empty in (m.calc_pred_logpdf(x[:0], k[:0], y[:0]), m.calc_pred_logpdf(x[:0], k[:0], y[:0], total=True)[0]):
        assert empty.shape == (0,) and empty.dtype == np.float64 and m._engine is None
    assert m.calc_pred_logpdf(x[:0], k[:0], y[:0], total=True)[1] == 0.0
    if not torch.cuda.is_available():          # (an unmarked test does not touch the device)
        with pytest.raises(EngineUnavailableError):
            m.calc_pred_logpdf(x, k, y)
        assert m._p_x is kept
