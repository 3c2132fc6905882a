"""The C-ABI library loads without a GPU and exports every symbol its five headers declare, at the pinned ABI versions;
the host-side seam the four small bindings share (bayesml_amd/_native.py)."""
import ctypes
import importlib
import os
import re

import pytest

from conftest import ROOT


def header_text(header):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)


def header_functions(header="gmmvb.h", prefix="gmmvb|hmmvb"):
    return sorted(set(re.findall(rf"\b((?:{prefix})_[a-z0-9_]+)\s*\(", header_text(header))))


def test_header_declares_the_expected_entry_points():
    names = header_functions()
    for must in ("gmmvb_workspace_create", "gmmvb_workspace_destroy", "gmmvb_set_params", "gmmvb_estep",
                 "gmmvb_mstep", "gmmvb_estep_mstep", "gmmvb_responsibilities", "gmmvb_argmax", "gmmvb_stats_len"):
        assert must in names


# ---- what each family checks beside the table and the version: its length functions and the limits its binding repeats ----
def _gmmvb_also(lib, mod, text):
    assert lib.gmmvb_stats_len(64, 128) == 64 * (2 + 128 + 128 * 128)
    assert lib.gmmvb_stats_len(0, 4) == -1
    assert lib.gmmvb_stats_packed_len(64, 128) == 64 * (2 + 128 + 128 * 129 // 2)
    assert lib.gmmvb_stats_packed_len(3, 0) == -1


def _regvb_also(lib, mod, text):
    assert lib.regvb_stats_len(128) == 128 * 128 + 128 + 2
    assert lib.regvb_stats_len(0) == -1 and lib.regvb_stats_len(257) == -1
    assert lib.regvb_stats_work_len(128) > 0 and lib.regvb_predict_work_len(256) == 128 * 16 * 17
    assert lib.regvb_stats_work_len(300) == -1 and lib.regvb_predict_work_len(0) == -1


def _expfam_also(lib, mod, text):
    assert mod.MAX_DEGREE == int(re.search(r"#define EXPFAM_MAX_DEGREE (\d+)", text).group(1))


def _ctree_also(lib, mod, text):
    assert "ctree_" not in header_text("gmmvb.h")


def _mtree_also(lib, mod, text):
    for name, value in (("MTREE_MAX_TREES", mod.MAX_TREES), ("MTREE_MAX_NODES", mod.MAX_NODES),
                        ("MTREE_MAX_CHILDREN", mod.MAX_CHILDREN), ("MTREE_MAX_DEGREE", mod.MAX_DEGREE),
                        ("MTREE_MAX_DEPTH", mod.MAX_DEPTH), ("MTREE_MAX_SLABS", mod.MAX_SLABS),
                        ("MTREE_LDS_SLOTS", mod.LDS_SLOTS)):
        assert re.search(rf"#define {name} {value}\b", text), name


ABIS = [("gmmvb.h", "gmmvb|hmmvb", "_engine", 8, _gmmvb_also), ("regvb.h", "regvb", "_regression", 1, _regvb_also),
        ("expfam.h", "expfam", "_expfam", 1, _expfam_also), ("ctree.h", "ctree", "_ctree", 1, _ctree_also),
        ("mtree.h", "mtree", "_mtree", 2, _mtree_also)]


@pytest.mark.parametrize("header, prefix, module, version, also", ABIS, ids=[a[0][:-2] for a in ABIS])
def test_library_exports_every_declared_symbol(header, prefix, module, version, also):
    """Header <-> .so <-> ctypes table, and the ABI version pinned in all three places."""
    from bayesml_amd import _engine
    if not os.path.exists(_engine.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    mod = importlib.import_module("bayesml_amd." + module)
    lib = mod.load_library()
    declared = header_functions(header, prefix)
    assert sorted(mod.SYMBOLS) == declared, "ctypes table and header disagree"
    for name in declared:
        assert getattr(lib, name) is not None
    family = prefix.split("|")[0]
    text = header_text(header)
    in_header = int(re.search(rf"#define {family.upper()}_ABI_VERSION (\d+)", text).group(1))
    assert getattr(lib, family + "_abi_version")() == version == in_header
    also(lib, mod, text)


def test_argument_errors_without_a_gpu():
    """Pure argument validation returns error codes (no compute, no device needed)."""
    import ctypes
    from bayesml_amd import _engine
    lib = _engine.load_library()
    h = ctypes.c_void_p()
    assert lib.gmmvb_workspace_create(0, 4, 0, 10, ctypes.byref(h)) == 1          # GMMVB_EINVAL
    assert lib.gmmvb_workspace_create(4, 4, 0, 0, ctypes.byref(h)) == 1
    assert lib.gmmvb_workspace_create(4, 4, 7, 10, ctypes.byref(h)) == 1
    assert b"x_dtype" in lib.gmmvb_last_error()
    assert lib.gmmvb_workspace_destroy(None) == 0


def test_product_path_fails_loudly_without_gpu():
    import numpy as np
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from bayesml_amd import gaussianmixture as gm
    from bayesml_amd._engine import EngineUnavailableError
    m = gm.LearnModel(3, 2, seed=0)
    with pytest.raises(EngineUnavailableError):
        m.update_posterior(np.zeros((10, 2)))
    with pytest.raises(EngineUnavailableError):
        m.estimate_latent_vars(np.zeros((10, 2)))


# ---- the seam of the four small bindings (bayesml_amd/_native.py) ------------------------------------------------------
P = ctypes.c_void_p(4096)           # never dereferenced: every call below is refused on its arguments


def _refused(family):
    """(module, a call the library refuses, the entry point's name, the EngineError text the binding raises for it)."""
    from bayesml_amd import _ctree, _expfam, _mtree, _regression
    return {
        "regvb": (_regression, lambda lib: lib.regvb_stats(0, 0, P, 4, 0, P, 10, P, P, None), "regvb_stats",
                  "regvb_stats: GMMVB_EINVAL: regvb_stats: D must be >= 1"),
        "expfam": (_expfam, lambda lib: lib.expfam_stats_counts(_expfam.I32, P, 10, 0, P, P, None), "expfam_stats_counts",
                   "expfam_stats_counts: GMMVB_EINVAL: expfam_stats_counts: degree must be >= 1"),
        "ctree": (_ctree, lambda lib: lib.ctree_count(_ctree.U8, P, 10, 0, 2, P, P, None), "ctree_count",
                  "ctree_count: GMMVB_EINVAL: ctree_count: k and D must be >= 1"),
        "mtree": (_mtree, lambda lib: lib.mtree_stat_cols(_mtree.CATEGORICAL, 17, None, None, None), "mtree_stat_cols",
                  "mtree_stat_cols: GMMVB_EUNSUPPORTED: mtree_stat_cols: a categorical degree above 16 is not supported"),
    }[family]


FAMILIES = ("regvb", "expfam", "ctree", "mtree")


@pytest.mark.parametrize("family", FAMILIES)
def test_check_raises_the_family_s_own_message(family):
    from bayesml_amd._engine import EngineError
    mod, call, what, text = _refused(family)
    mod._check(0, what)
    with pytest.raises(EngineError) as e:
        mod._check(call(mod.load_library()), what)
    assert str(e.value) == text


def test_an_error_in_one_family_leaves_the_others_messages():
    lib = None
    for family in FAMILIES:
        mod, call, _, _ = _refused(family)
        lib = mod.load_library()
        assert call(lib) != 0
    for family in FAMILIES:          # every slot still holds its own family's message, the first after three later failures
        text = _refused(family)[3]
        assert getattr(lib, family + "_last_error")().decode() == text.split(": ", 2)[2]


def test_bind_declares_a_table_once():
    from bayesml_amd import _ctree, _engine, _native

    class Counting(dict):
        reads = 0

        def items(self):
            Counting.reads += 1
            return super().items()

    load, _ = _native.bind("ctree", Counting(ctree_abi_version=(ctypes.c_int, [])))
    assert Counting.reads == 0
    lib = load()
    assert lib is _engine.load_library() and Counting.reads == 1
    assert load() is lib and Counting.reads == 1
    assert _ctree.load_library() is lib is _ctree.load_library()
    with pytest.raises(AttributeError):
        _native.bind("ctree", {"ctree_no_such_entry_point": (ctypes.c_int, [])})[0]()


def test_gpu_device_refuses_anything_but_a_gpu():
    import torch
    from bayesml_amd import _native
    from bayesml_amd._engine import EngineUnavailableError
    if torch.cuda.is_available():
        return                              # (an unmarked test does not touch the device)
    for what, text in (("regression data passes", "bayesml_amd's regression data passes need an MI355X: there is no CPU fallback"),
                       ("meta-tree engine", "bayesml_amd's meta-tree engine needs an MI355X: there is no CPU fallback")):
        with pytest.raises(EngineUnavailableError) as e:
            _native.gpu_device(None, what)
        assert str(e.value) == text
