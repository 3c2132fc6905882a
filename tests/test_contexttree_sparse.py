"""contexttree with tables="sparse", without a GPU: the constructor and its limits, the argument checks and sizes of the
ctsp_* entry points, header <-> library <-> ctypes table, and the sparse oracle against the reference's fixtures."""
import ctypes
import os
import re

import numpy as np
import pytest

import contexttree_sparse_oracle as sorc
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c["name"] for c in sorc.CASES]


def _ct():
    from bayesml_amd import contexttree
    return contexttree


def test_tables_keyword():
    """Fails without the feature: the keyword does not exist on the parent commit."""
    from bayesml_amd._engine import EngineLimitError
    from bayesml_amd._exceptions import ParameterFormatError
    ct = _ct()
    m = ct.LearnModel(4, 12, tables="sparse")
    assert m.hn_root is None and m.get_constants() == {"c_k": 4, "c_d_max": 12}
    with pytest.raises(EngineLimitError):
        ct.LearnModel(4, 12, tables="dense")
    with pytest.raises(EngineLimitError):
        ct.LearnModel(4, 12)
    with pytest.raises(ParameterFormatError):
        ct.LearnModel(4, 12, tables="other")
    assert not ct.LearnModel(2, 3)._sparse and ct.LearnModel(2, 3, tables="dense")._engine is None


def test_sparse_limits():
    from bayesml_amd import _ctsp
    from bayesml_amd._engine import EngineLimitError
    ct = _ct()
    for k, d in ((256, 7), (16, 15), (4, 31), (3, 31), (2, 63), (5, 21), (1, 63), (129, 7)):
        ct.LearnModel(k, d, tables="sparse")
        assert _ctsp.load_library().ctsp_key_bits(k, d) == _ctsp.symbol_bits(k) * d <= 63
    for k, d in ((2, 64), (4, 32), (3, 32), (256, 8), (16, 16), (5, 22), (257, 1), (1, 64)):
        with pytest.raises(EngineLimitError):
            ct.LearnModel(k, d, tables="sparse")
        assert _ctsp.load_library().ctsp_key_bits(k, d) == -1


def test_no_gpu_means_unavailable():
    import torch
    from bayesml_amd import _ctsp
    from bayesml_amd._engine import EngineUnavailableError
    if not torch.cuda.is_available():
        with pytest.raises(EngineUnavailableError):
            _ct().LearnModel(4, 12, tables="sparse").update_posterior(np.array([0, 1, 1]))
        with pytest.raises(EngineUnavailableError):
            _ctsp.SparseCtreePass(4, 12)


def test_key_helpers():
    from bayesml_amd import _ctsp
    assert [_ctsp.symbol_bits(k) for k in (1, 2, 3, 4, 5, 16, 17, 256)] == [1, 1, 2, 2, 3, 4, 5, 8]
    lib = _ctsp.load_library()
    assert all(lib.ctsp_symbol_bits(k) == _ctsp.symbol_bits(k) for k in range(1, 257))
    assert lib.ctsp_symbol_bits(0) == -1 and lib.ctsp_symbol_bits(257) == -1
    k, D = 3, 5
    key = _ctsp.key_of([2, 0, 1], k, D)
    assert key == (2 << 8) | (0 << 6) | (1 << 4) == sorc.pack([2, 0, 1], k, D)
    assert _ctsp.context_of(key, 3, k, D) == [2, 0, 1] == sorc.unpack(key, 3, k, D)
    assert _ctsp.parent_key(key, 3, k, D) == _ctsp.key_of([2, 0], k, D)
    assert _ctsp.child_key(_ctsp.key_of([2, 0], k, D), 2, 1, k, D) == key
    assert _ctsp.key_of([], k, D) == 0
    # the widest keys stay below bit 63, so the all-ones word is never a key
    assert _ctsp.key_of([1] * 63, 2, 63) == 2 ** 63 - 1 and _ctsp.key_of([255] * 7, 256, 7) == 2 ** 56 - 1


def test_sizes_and_argument_errors_without_a_gpu():
    """Pure argument validation: status codes and messages, nothing touches a device."""
    from bayesml_amd import _ctsp
    lib = _ctsp.load_library()
    EINVAL, EUNSUP = 1, 2
    assert lib.ctsp_slot_bytes(4) == 8 + 32 + 8 + 2 + 32 + 8 and lib.ctsp_slot_bytes(256) == 4096 + 26
    assert lib.ctsp_slot_bytes(0) == -1 and lib.ctsp_slot_bytes(257) == -1
    # capacity: the smallest power of two >= 2 (present + min(n, k^level)), need capped at k^level, never below the floor
    assert lib.ctsp_capacity(4, 12, 0, 0, 1500, 0) == 2 and lib.ctsp_capacity(4, 12, 1, 0, 1500, 0) == 8
    assert lib.ctsp_capacity(4, 12, 12, 0, 1500, 0) == 4096 and lib.ctsp_capacity(4, 12, 12, 1400, 700, 0) == 8192
    assert lib.ctsp_capacity(4, 12, 12, 1024, 1024, 0) == 4096 and lib.ctsp_capacity(4, 12, 12, 1024, 1025, 0) == 8192
    assert lib.ctsp_capacity(4, 12, 2, 16, 1500, 0) == 32 and lib.ctsp_capacity(4, 12, 3, 0, 0, 64) == 64
    assert lib.ctsp_capacity(2, 63, 63, 0, 10 ** 7, 0) == 2 ** 25 and lib.ctsp_capacity(1, 5, 3, 0, 100, 0) == 2
    for bad in ((0, 3, 0, 0, 1, 0), (2, 0, 0, 0, 1, 0), (2, 3, 4, 0, 1, 0), (2, 3, -1, 0, 1, 0), (2, 64, 0, 0, 1, 0),
                (257, 1, 0, 0, 1, 0), (2, 3, 0, -1, 1, 0), (2, 3, 0, 0, -1, 0), (2, 3, 0, 0, 1, -1)):
        assert lib.ctsp_capacity(*bad) == -1
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4097)       # never dereferenced: every call fails its checks first
    off = (ctypes.c_int64 * 4)(0, 2, 6, 14)                     # D = 2
    not_pow2 = (ctypes.c_int64 * 4)(0, 2, 5, 13)
    not_zero = (ctypes.c_int64 * 4)(2, 4, 8, 16)
    wide = (ctypes.c_int64 * 66)(*range(0, 132, 2))

    def msg():
        return lib.ctsp_last_error().decode()
    assert lib.ctsp_count(0, p, 10, 2, 64, wide, p, p, p, p, None) == EUNSUP and "not supported" in msg()
    assert lib.ctsp_count(0, p, 10, 257, 1, wide, p, p, p, p, None) == EUNSUP
    assert lib.ctsp_count(0, p, 10, 0, 2, off, p, p, p, p, None) == EINVAL and "k and D" in msg()
    assert lib.ctsp_count(3, p, 10, 2, 2, off, p, p, p, p, None) == EINVAL and "dtype" in msg()
    assert lib.ctsp_count(0, p, 0, 2, 2, off, p, p, p, p, None) == EINVAL and "n must be >= 1" in msg()
    assert lib.ctsp_count(0, None, 5, 2, 2, off, p, p, p, p, None) == EINVAL and "null" in msg()
    assert lib.ctsp_count(0, p, 5, 2, 2, off, p, p, p, None, None) == EINVAL and "null" in msg()
    assert lib.ctsp_count(0, p, 5, 2, 2, None, p, p, p, p, None) == EINVAL and "null" in msg()
    assert lib.ctsp_count(0, p, 5, 2, 2, not_pow2, p, p, p, p, None) == EINVAL and "power of two" in msg()
    assert lib.ctsp_count(0, p, 5, 2, 2, not_zero, p, p, p, p, None) == EINVAL and "off[0]" in msg()
    assert lib.ctsp_count(1, odd, 5, 2, 2, off, p, p, p, p, None) == EINVAL and "aligned" in msg()
    assert lib.ctsp_count(0, p, 5, 2, 2, off, odd, p, p, p, None) == EINVAL and "aligned" in msg()
    assert lib.ctsp_levelup(2, 64, wide, p, p, p, 0, p, None) == EUNSUP
    assert lib.ctsp_levelup(2, 2, off, p, p, p, 3, p, None) == EINVAL and "n_head" in msg()
    assert lib.ctsp_levelup(2, 2, off, p, p, None, 1, p, None) == EINVAL and "null" in msg()
    assert lib.ctsp_levelup(2, 2, not_pow2, p, p, p, 1, p, None) == EINVAL and "power of two" in msg()
    assert lib.ctsp_levelup(2, 2, off, p, odd, p, 1, p, None) == EINVAL and "misaligned" in msg()
    sweep_ok = [2, 2, off, p, p, p, p, p, p, p, p, 1, 0.5, p, None]

    def sweep(**kw):
        a = list(sweep_ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.ctsp_sweep(*a)
    assert sweep(a1=64, a2=wide) == EUNSUP and sweep(a1=0) == EINVAL
    assert sweep(a11=3) == EINVAL and "n_head" in msg()
    assert sweep(a10=None) == EINVAL and "null" in msg()
    assert sweep(a9=None) == EINVAL and "null" in msg()
    assert sweep(a12=1.5) == EINVAL and "hn_g" in msg()
    assert sweep(a12=float("nan")) == EINVAL and "hn_g" in msg()
    assert sweep(a6=odd) == EINVAL and "misaligned" in msg()
    assert sweep(a2=not_pow2) == EINVAL and "power of two" in msg()
    assert lib.ctsp_map(2, 64, wide, p, p, p, 0.5, p, p, None) == EUNSUP
    assert lib.ctsp_map(2, 2, off, p, None, p, 0.5, p, p, None) == EINVAL and "null" in msg()
    assert lib.ctsp_map(2, 2, off, p, p, p, -0.1, p, p, None) == EINVAL and "hn_g" in msg()
    assert lib.ctsp_map(2, 2, off, p, odd, p, 0.5, p, p, None) == EINVAL and "misaligned" in msg()
    assert lib.ctsp_find(2, 64, wide, p, 1, p, p, 0, p, p, None) == EUNSUP
    assert lib.ctsp_find(2, 2, off, p, 0, p, p, 0, p, p, None) == EINVAL and "nq" in msg()
    assert lib.ctsp_find(2, 2, off, p, 1, None, p, 0, p, p, None) == EINVAL and "null" in msg()
    assert lib.ctsp_find(2, 2, off, p, 1, p, odd, 0, p, p, None) == EINVAL and "misaligned" in msg()
    assert lib.ctsp_rehash(2, 64, wide, p, p, p, p, p, wide, p, p, p, p, p, p, None) == EUNSUP
    q = ctypes.c_void_p(8192)
    assert lib.ctsp_rehash(2, 2, off, p, p, p, p, p, off, q, None, q, q, q, p, None) == EINVAL and "null" in msg()
    assert lib.ctsp_rehash(2, 2, off, p, p, p, p, p, not_pow2, q, q, q, q, q, p, None) == EINVAL and "power of two" in msg()
    assert lib.ctsp_rehash(2, 2, off, p, p, p, p, p, off, p, q, q, q, q, p, None) == EINVAL and "differ" in msg()
    assert lib.ctsp_rehash(2, 2, off, p, p, p, p, p, off, q, odd, q, q, q, p, None) == EINVAL and "misaligned" in msg()


def test_header_library_and_ctypes_table_agree():
    from bayesml_amd import _ctsp
    text = open(os.path.join(ROOT, "include", "ctsp.h")).read()
    body = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(ctsp_[a-z_]+)\s*\(", body))
    assert declared == set(_ctsp.SYMBOLS)
    lib = _ctsp.load_library()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.ctsp_abi_version() == 1 == int(re.search(r"#define CTSP_ABI_VERSION (\d+)", text).group(1))
    assert int(re.search(r"#define CTSP_MAX_K (\d+)", text).group(1)) == _ctsp.MAX_K
    assert int(re.search(r"#define CTSP_MAX_KEY_BITS (\d+)", text).group(1)) == _ctsp.MAX_KEY_BITS
    # argument counts of the prototypes against the ctypes table
    for name, (_, args) in _ctsp.SYMBOLS.items():
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, body).group(1).strip()
        n_args = 0 if proto == "void" else proto.count(",") + 1
        assert n_args == len(args), name


@pytest.mark.parametrize("name", NAMES)
def test_fixture_inputs_are_the_seeded_recipe(name):
    fx, inp = load_golden(f"contexttree_sparse_{name}.npz"), sorc.case_inputs(sorc.case_by_name(name))
    for key, a in inp.items():
        assert np.array_equal(fx[key], a), key
    assert int(fx["map_stored"]) == int(sorc.case_by_name(name)["map_stored"]) == int("map_level" in fx)


@pytest.mark.parametrize("name", NAMES)
def test_sparse_oracle_matches_reference(name):
    """The batch form on node dictionaries against the reference's sequential update: node set, h_beta_vec and leaf
    exactly, h_g in log-odds to the ref_vs_batch that the generator recorded for the case."""
    case = sorc.case_by_name(name)
    fx, inp = load_golden(f"contexttree_sparse_{name}.npz"), sorc.case_inputs(case)
    stages = sorc.oracle_stages(case, inp, sorc.stage_lists(fx, "prior") if case["h0root"] else None)
    assert ("after2" in stages) == (case["n2"] > 0) == ("after2_level" in fx)
    for stage, t in stages.items():
        ref = sorc.stage_lists(fx, stage)
        assert sorc.same_node_set(t, ref)
        assert np.array_equal(t["beta"], ref["beta"]) and np.array_equal(t["leaf"], ref["leaf"])
        assert sorc.g_err(t, ref) <= float(fx["ref_vs_batch"])


def test_sparse_oracle_agrees_with_the_dense_oracle():
    """Where both run, the node-dictionary form and the dense-table form are the same arithmetic."""
    import contexttree_oracle as orc
    rng = np.random.default_rng(5)
    for k, D, n in ((2, 3, 200), (3, 4, 300), (5, 1, 50), (4, 3, 2)):
        x1, x2 = rng.integers(0, k, n), rng.integers(0, k, max(1, n // 3))
        hb = np.arange(1, k + 1) / 2.0
        t, nodes = orc.new_tables(k, D), {}
        for x in (x1, x2):
            orc.batch_update(x, k, D, t, 0.4, hb)
            sorc.batch_update(x, k, D, nodes, 0.4, hb)
        lists = sorc.nodes_to_lists(nodes, k, D)
        idx = [orc.path_indices(c[:d], k, D)[-1] for d, c in zip(lists["level"], lists["ctx"])]
        assert len(idx) == int(t["exists"].sum()) and np.all(t["exists"][idx] == 1)
        assert np.array_equal(t["beta"][idx], lists["beta"]) and np.array_equal(t["leaf"][idx], lists["leaf"])
        np.testing.assert_allclose(t["g"][idx], lists["g"], rtol=1e-12, atol=0)
