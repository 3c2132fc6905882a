"""The workspace's switches, shape, buffer list and life cycle (bayesml_amd/csrc/workspace_plan.h) without a GPU.

tests/workspace_plan_cases.cpp includes only that header; it is built here by the host compiler with AddressSanitizer and
UBSan and run once over every case below.  What it answers is compared with what create_workspace and ensure_lists of
capi.hip did before the life cycle was moved out of them: ``parent_options`` and ``parent_workspace`` below are those two
functions written out expression by expression.  The totals are also held against gmmvb_workspace_bytes as that code
reported it on an MI355X (256 CUs), less what its hand-written formula miscounted (profiles/workspace.md).

Kernel sizes are literals.  They were printed once by a few lines of host code linked against libgmmvb.so (the launch.h
functions of the same names; slab_len and generic_rows from common.h / generic.h) for T = 1, 3, 4, 8, 10 and the D below;
T = 19 (D = 300) is generic and uses none of them."""
import os
import subprocess

import pytest

from test_pass_plan import HERE, host_compiler

CONSTANTS = dict(max_tiles=8, t1_splits=24, sel_rows=256, lse_rows=1024, scan_parts=1024, rec_slots=8, estep_tri_image_doubles=160)
BY_T = {1: dict(mstep_components_per_wg=4, estep_image_doubles=384, estep_bound_blocks=0, slab_len=288),
        3: dict(mstep_components_per_wg=4, estep_image_doubles=1664, estep_bound_blocks=0, slab_len=1600),
        4: dict(mstep_components_per_wg=4, estep_image_doubles=2688, estep_bound_blocks=2, slab_len=2640),
        8: dict(mstep_components_per_wg=2, estep_image_doubles=9344, estep_bound_blocks=3, slab_len=9360),
        10: dict(mstep_components_per_wg=1, estep_image_doubles=14336, estep_bound_blocks=3, slab_len=14256)}
BY_D = {8: (7168, 4096, 96), 16: (7168, 4096, 96), 48: (19456, 10240, 192), 49: (19456, 10240, 192), 64: (19456, 10240, 192),
        128: (63488, 31744, 384), 160: (95232, 47104, 480)}      # estep_i8_image_bytes(D, 0), (D, 1), estep_i8_digit_row_bytes(D)
PROJ = {(1, 8): (2048, 32), (4, 16): (8192, 128), (6, 48): (24576, 192), (6, 49): (24576, 192), (8, 64): (32768, 256),
        (8, 128): (65536, 256), (257, 64): (9474048, 74016), (4, 160): (40960, 128), (6, 64): (24576, 192), (1, 160): (10240, 32),
        (2, 64): (8192, 64)}                                     # proj_image_len(K, D), proj_const_len(K)


def kernel_sizes(K, D):
    ks = dict(CONSTANTS, generic_rows=64)
    if D > 256:
        return ks
    T = (D + 15) // 16
    ks.update(BY_T[T + T % 2 if D > 128 else T])
    ks.update(zip(("estep_i8_image_bytes", "estep_i8_bound_image_bytes", "estep_i8_digit_row_bytes"), BY_D[D]))
    ks.update(zip(("proj_image_len", "proj_const_len"), PROJ[K, D]))
    return ks


# ---- the parent's create_workspace, line by line ---------------------------------------------------------------------------
DEFAULTS = dict(sparse=1, prune=1, variant_asked=-1, sort_rows=1, settle_margin=1e300, opt_proof=1, opt_proof_all=1,
                opt_proof_blocked=1, opt_lazy=1, opt_project=0, opt_regroup_margin=1, gather_exit=1, cache_on=1, opt_carry_off=0,
                opt_hmm_mstep_dense=0, opt_calibrate=1, opt_debug=0, opt_mlist_xc=0)
LDS, DIRECT, LDS8, I8, VALU16 = 0, 1, 2, 3, 4


def parent_options(env):
    dbg = env.get("GMMVB_DEBUG")
    dev = (lambda name: env.get(name)) if dbg and dbg[0] != "0" else (lambda name: None)      # dev_env
    not_zero = lambda v: int(not (v is not None and v == "0"))      # noqa: E731   !(v && strcmp(v, "0") == 0)
    o = dict(DEFAULTS)
    o["sparse"] = not_zero(env.get("GMMVB_MSTEP_SPARSE"))
    v = env.get("GMMVB_ESTEP_PRUNE")
    o["prune"] = 0 if v == "0" else (2 if v == "force" else 1)
    o["variant_asked"] = {"lds8": LDS8, "direct": DIRECT, "lds4": LDS, "i8": I8}.get(dev("GMMVB_ESTEP_VARIANT"), -1)
    o["sort_rows"] = not_zero(dev("GMMVB_SORT_ROWS"))
    if dev("GMMVB_SETTLE_MARGIN") is not None:
        o["settle_margin"] = float(dev("GMMVB_SETTLE_MARGIN"))
    o["opt_proof"] = not_zero(dev("GMMVB_PROOF"))
    o["opt_proof_all"] = int(dev("GMMVB_PROOF") != "settled")
    o["opt_proof_blocked"] = not_zero(dev("GMMVB_PROOF_BLOCKED"))
    o["opt_lazy"] = not_zero(dev("GMMVB_SWEEP_LAZY"))
    o["opt_project"] = {"filter": 1, "only": 2}.get(dev("GMMVB_PROJECT"), 0)
    o["opt_regroup_margin"] = not_zero(dev("GMMVB_REGROUP_MARGIN"))
    o["gather_exit"] = not_zero(dev("GMMVB_GATHER_EXIT"))
    o["cache_on"] = not_zero(dev("GMMVB_MSTEP_CACHE"))
    o["opt_carry_off"] = int(dev("GMMVB_ESTEP_CARRY_OFF") is not None)
    o["opt_hmm_mstep_dense"] = int(dev("GMMVB_HMM_MSTEP_DENSE") is not None)
    o["opt_calibrate"] = not_zero(dev("GMMVB_POLICY_CALIBRATE"))
    o["opt_debug"] = int(dbg is not None and dbg[:1] == "2")
    # (gmmvb_mstep read this one, at its first list pass: dev_env(..) && dev_env(..)[0] == '1')
    o["opt_mlist_xc"] = int(dev("GMMVB_MLIST_XC") is not None and dev("GMMVB_MLIST_XC")[:1] == "1")
    return o


def round_up(v, m):
    return (v + m - 1) // m * m


ZERO, PINNED, SCRATCH, ZERO_LAST = 1, 2, 4, 8      # (ZERO_LAST: zeroed once everything is allocated)


def parent_workspace(K, D, f64, max_rows, env, num_cu=256):
    """(shape fields, the switches in force, [(buffer, bytes, flags)] in the order of allocation) as the parent made them."""
    ks = kernel_sizes(K, D)
    T = (D + 15) // 16
    wide = 128 < D <= 256
    if wide:
        T = 2 * ((T + 1) // 2)
    npad = round_up(max_rows, 64)
    bufs = []
    add = lambda name, n, flags=0: bufs.append((name, n, flags)) if n else None      # noqa: E731
    if D > 256:
        gen_S = min(64, max(1, max_rows // 16384))
        shape = dict(T=T, wide=0, generic=1, npad=npad, KG=0, S_cap=0, split_rows=0, img_len=0, variant=0, gen_S=gen_S, lists=0)
        on = dict(DEFAULTS, sparse=0, prune=0, sort_rows=0, cache_on=0)
        for name, n, fl in (("lnrho", K * npad, SCRATCH), ("lse", npad, 0), ("cvec", K, 0), ("pivot", D, ZERO_LAST), ("gen_u", K * D * D, 0),
                            ("gen_m", K * D, 0), ("gen_first", gen_S * K * (D + 2), 0),
                            ("gen_second", gen_S * K * (T * (T + 1) // 2) * 256, 0), ("ctr", 8, ZERO_LAST)):
            add(name, 8 * n, fl)
        add("ctr_host", 64, PINNED)
        return shape, on, bufs
    on = parent_options(env)
    KG = (K + ks["mstep_components_per_wg"] - 1) // ks["mstep_components_per_wg"]
    S_cap = round_up(((24 if T == 1 else 4) * num_cu + KG - 1) // KG, 8)
    S_cap = max(S_cap, 8)
    split_rows = round_up(max(64, (16 << 20) // (16 * T * 8)), 64)
    S_cap = max(S_cap, round_up((max_rows + split_rows - 1) // split_rows, 8))
    variant = VALU16 if T == 1 else LDS8
    if not wide and on["variant_asked"] >= 0:
        variant = on["variant_asked"]
    if variant == VALU16:
        add("tri", K * 160 * 8)
    xc_len = (npad + 64) * 16 * T
    if max_rows > 2000000000 or wide:
        on["sparse"] = 0
    if K == 1:
        on["sparse"] = 0
        if not wide:
            xc_len = 0
    on["sort_rows"] = int(on["sort_rows"] and max_rows <= 2000000000)
    if not on["sparse"] or ks["estep_bound_blocks"] == 0 or K > 256:
        on["prune"] = 0
    full, bound = variant == I8, on["prune"] != 0
    if full:
        add("img_i8", K * ks["estep_i8_image_bytes"])
    if bound:
        add("img_i8b", K * ks["estep_i8_bound_image_bytes"])
    if full or bound:
        add("pivot_i8", D * 8)
    blocks = (npad + 255) // 256
    for name, n, fl in (("lnrho", K * npad, SCRATCH), ("lse", npad, 0), ("img", K * ks["estep_image_doubles"], 0), ("cvec", K, 0),
                        ("pivot", D, ZERO_LAST), ("slabs", S_cap * K * ks["slab_len"], SCRATCH), ("xc", xc_len, SCRATCH),
                        ("dpart", (npad + 1023) // 1024 * K, 0), ("thr", K, 0), ("apart", blocks, 0), ("ctr", 8, ZERO_LAST), ("drift", 4 * K, 0)):
        add(name, 8 * n, fl)
    lists = bool(on["sparse"] and K <= 256)
    if lists:                                    # ensure_lists
        words = (K + 63) // 64
        add("lists", K * npad * 4, SCRATCH)
        add("khat", npad * 4)
        add("counts", K * 4)
        add("plan", (K + 1) * 4)
        add("plan_m", (K + 2) * 4)
        add("blk", blocks * K * 4)
        add("scan_parts", K * 1024 * 4)
        add("masks", words * npad * 8)
        add("lock", npad, ZERO)
        add("lcomp", npad)
        add("dlock", npad * 4)
        add("rthr", npad * 4)
        add("exit_ctr", 32, ZERO)
        add("exit_host", 32, PINNED | ZERO)
        add("dmask", words * npad * 8)
        add("dblk", blocks * K * 4)
        add("mmask", words * npad * 8)
        add("rmask", words * npad * 8)
        add("rblk", blocks * K * 4)
        add("mblk", blocks * K * 4)
        add("cache", K * (2 + D + D * D) * 8, ZERO)
        for name in ("spart", "gpart", "qpart", "epart", "opart", "mpart"):
            add(name, blocks * 8)
        add("ppart", blocks * 8, ZERO)
        if on["prune"] != 0 and on["opt_proof"] and on["cache_on"]:
            add("xq", npad * ks["estep_i8_digit_row_bytes"])
            add("xqe", npad)
            if on["opt_project"] != 0 and on["sort_rows"] and K <= 256 and 32 < D <= 128:
                add("gimg", ks["proj_image_len"], ZERO)
                add("gconst", ks["proj_const_len"] * 16)
                add("tile_ref", blocks * 4)
        add("rec_k", 8 * npad * 2)
        add("rec_d", 8 * npad * 4)
        add("rec_B", npad * 4)
        for name in ("rec_exact", "rec_sel", "rec_flags"):
            add(name, npad)
        add("ub32", K * npad * 4)
        if on["opt_lazy"] and K <= 256:
            add("tmeta", blocks * K * 16)
        if on["sort_rows"]:
            add("xp", max_rows * D * (8 if f64 else 4))
            for name in ("perm", "iperm", "perm_tmp"):
                add(name, npad * 4)
    add("ctr_host", 64, PINNED)
    shape = dict(T=T, wide=int(wide), generic=0, npad=npad, KG=KG, S_cap=S_cap, split_rows=split_rows, img_len=ks["estep_image_doubles"],
                 variant=variant, gen_S=1, lists=int(lists))
    return shape, on, bufs


# ---- cases -------------------------------------------------------------------------------------------------------------------
DBG = {"GMMVB_DEBUG": "1"}
DEV_SWITCHES = ["GMMVB_SORT_ROWS", "GMMVB_PROOF", "GMMVB_PROOF_BLOCKED", "GMMVB_SWEEP_LAZY", "GMMVB_REGROUP_MARGIN", "GMMVB_GATHER_EXIT",
                "GMMVB_MSTEP_CACHE", "GMMVB_POLICY_CALIBRATE", "GMMVB_ESTEP_CARRY_OFF", "GMMVB_HMM_MSTEP_DENSE", "GMMVB_PROJECT",
                "GMMVB_ESTEP_VARIANT", "GMMVB_SETTLE_MARGIN"]
# (environment, what differs from DEFAULTS) - read off the parent's create_workspace; parent_options must agree
OPTIONS = [({}, {})]
OPTIONS += [({"GMMVB_MSTEP_SPARSE": v}, {"sparse": s}) for v, s in (("0", 0), ("1", 1), ("force", 1))]
OPTIONS += [({"GMMVB_ESTEP_PRUNE": v}, {"prune": p}) for v, p in (("0", 0), ("1", 1), ("force", 2), ("settled", 1))]
OPTIONS += [({"GMMVB_DEBUG": v}, {"opt_debug": d}) for v, d in (("0", 0), ("1", 0), ("2", 1))]
for name, field in (("GMMVB_SORT_ROWS", "sort_rows"), ("GMMVB_PROOF_BLOCKED", "opt_proof_blocked"), ("GMMVB_SWEEP_LAZY", "opt_lazy"),
                    ("GMMVB_REGROUP_MARGIN", "opt_regroup_margin"), ("GMMVB_GATHER_EXIT", "gather_exit"),
                    ("GMMVB_MSTEP_CACHE", "cache_on"), ("GMMVB_POLICY_CALIBRATE", "opt_calibrate")):
    OPTIONS += [(dict(DBG, **{name: "0"}), {field: 0}), (dict(DBG, **{name: "1"}), {}), (dict(DBG, **{name: "force"}), {})]
for name, field in (("GMMVB_ESTEP_CARRY_OFF", "opt_carry_off"), ("GMMVB_HMM_MSTEP_DENSE", "opt_hmm_mstep_dense")):
    OPTIONS += [(dict(DBG, **{name: "0"}), {field: 1}), (dict(DBG, **{name: "1"}), {field: 1})]      # set at all
OPTIONS += [(dict(DBG, GMMVB_PROOF="0"), {"opt_proof": 0}), (dict(DBG, GMMVB_PROOF="1"), {}),
            (dict(DBG, GMMVB_PROOF="settled"), {"opt_proof_all": 0})]
OPTIONS += [(dict(DBG, GMMVB_PROJECT=v), {"opt_project": p}) for v, p in (("0", 0), ("1", 0), ("filter", 1), ("only", 2))]
OPTIONS += [(dict(DBG, GMMVB_ESTEP_VARIANT=v), {"variant_asked": e})
            for v, e in (("0", -1), ("1", -1), ("lds8", LDS8), ("direct", DIRECT), ("lds4", LDS), ("i8", I8), ("only", -1))]
OPTIONS += [(dict(DBG, GMMVB_SETTLE_MARGIN=v), {"settle_margin": m}) for v, m in (("2.5", 2.5), ("-1", -1.0), ("0", 0.0))]
OPTIONS += [(dict(DBG, GMMVB_MLIST_XC=v), {"opt_mlist_xc": on}) for v, on in (("1", 1), ("0", 0), ("", 0), ("force", 0))]
OPTIONS += [({"GMMVB_MLIST_XC": "1"}, {})]
# a developer switch is ignored without GMMVB_DEBUG (unset, "0", empty); the two interface switches are not
for dbg in ({}, {"GMMVB_DEBUG": "0"}, {"GMMVB_DEBUG": ""}):
    OPTIONS += [(dict(dbg, **{name: "0"}), {}) for name in DEV_SWITCHES]
    OPTIONS += [(dict(dbg, GMMVB_PROJECT="filter", GMMVB_ESTEP_VARIANT="i8", GMMVB_PROOF="settled", GMMVB_SETTLE_MARGIN="2.5"), {})]
    OPTIONS += [(dict(dbg, GMMVB_MSTEP_SPARSE="0", GMMVB_ESTEP_PRUNE="force"), {"sparse": 0, "prune": 2})]
OPTIONS += [(dict(GMMVB_DEBUG="2", GMMVB_SORT_ROWS="0"), {"sort_rows": 0, "opt_debug": 1})]

F32, F64 = 0, 1
GPU_SHAPES = [(1, 8, F32, 1000), (4, 16, F64, 5000), (6, 48, F32, 5000), (8, 64, F32, 5000), (8, 128, F32, 70000), (257, 64, F32, 2000),
              (4, 160, F32, 3000), (3, 300, F64, 2000), (6, 64, F32, 5000)]
GPU_ENVS = [{"GMMVB_MSTEP_SPARSE": "0"}, {"GMMVB_ESTEP_PRUNE": "0"}, {"GMMVB_ESTEP_PRUNE": "force"}] + [
    dict(DBG, **{k: v}) for k, v in (("GMMVB_SORT_ROWS", "0"), ("GMMVB_SWEEP_LAZY", "0"), ("GMMVB_MSTEP_CACHE", "0"), ("GMMVB_PROOF", "0"),
                                     ("GMMVB_PROJECT", "filter"), ("GMMVB_ESTEP_VARIANT", "i8"), ("GMMVB_POLICY_CALIBRATE", "0"))]
SHAPES = [s + ({},) for s in GPU_SHAPES] + [(8, 64, F32, 5000, env) for env in GPU_ENVS] + [
    (1, 160, F32, 1000, {}),                     # K == 1 and wide: the centred copy stays
    (2, 64, F32, 2000000001, {}),                # no 32-bit row numbers: no lists, no regrouping
    (6, 49, F32, 5000, {}),                      # T = 4: the first tile count with a bound pass (D = 48 above is the last without)
    (4, 16, F64, 5000, dict(DBG, GMMVB_ESTEP_VARIANT="direct")),      # no packed triangular images
    (4, 160, F32, 3000, dict(DBG, GMMVB_ESTEP_VARIANT="i8")),         # wide: the variant is not looked at
    (3, 300, F64, 40000, dict(DBG, GMMVB_SORT_ROWS="0", GMMVB_DEBUG="2")),      # generic: no switch is, gen_S = 2
]
# gmmvb_workspace_bytes of the parent commit on an MI355X (num_cu = 256), and of the group (6, 64, f32, 5000) + a tile of 3000
PARENT_BYTES = {(1, 8, F32, 1000): 14176728, (4, 16, F64, 5000): 58901004, (6, 48, F32, 5000): 43568636, (8, 64, F32, 5000): 93205292,
                (8, 128, F32, 70000): 307384860, (257, 64, F32, 2000): 97697472, (4, 160, F32, 3000): 121298112,
                (3, 300, F64, 2000): 3409832, (6, 64, F32, 5000): 71276860}
PARENT_BYTES_ENV = [89666464, 92147052, 93205292, 91864620, 93202732, 92229484, 92229484, 93242236, 93360940, 93205292]
PARENT_BYTES_TILE = 2204316


def correction(K, npad, lists):
    """What the parent's formula in ensure_lists miscounted: K ints too many for counts / plan / plan_m, an eighth per-block
    counter that is `apart` (counted with the first buffers), and exit_ctr's 32 bytes left out."""
    return 32 - 4 * K - 8 * ((npad + 255) // 256) if lists else 0


def line(kind, K, D, f64, max_rows, env):
    words = [kind, f"K={K}", f"D={D}", f"f64={f64}", f"max_rows={max_rows}", "num_cu=256"]
    words += [f"ks.{k}={v}" for k, v in kernel_sizes(K, D).items()] + [f"env.{k}={v}" for k, v in env.items()]
    return " ".join(words)


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("workspace_plan") / "workspace_plan_cases")
    subprocess.run(host_compiler() + ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                      os.path.join(HERE, "workspace_plan_cases.cpp"), "-o", exe], check=True)
    lines = ["options " + " ".join(f"env.{k}={v}" for k, v in env.items()) for env, _want in OPTIONS]
    lines += [line("shape", *s) for s in SHAPES] + [line("life", *s, {}) for s in GPU_SHAPES]
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)      # directly: no LD_PRELOAD
    assert run.returncode == 0 and run.stderr == "", run.stderr
    out = run.stdout.splitlines()
    assert len(out) == len(lines), run.stdout
    return out[:len(OPTIONS)], out[len(OPTIONS):len(OPTIONS) + len(SHAPES)], out[len(OPTIONS) + len(SHAPES):]


def fields(text):
    return {kv.split("=")[0]: float(kv.split("=")[1]) for kv in text.split()}


def test_options(answers):
    wrong = []
    for (env, differs), have in zip(OPTIONS, answers[0]):
        want = dict(DEFAULTS, **differs)
        assert parent_options(env) == want, env          # the two readings of the parent agree
        wrong += [(env, k, v, fields(have)[k]) for k, v in want.items() if fields(have)[k] != v]
    assert not wrong, wrong


def test_shape_and_plan(answers):
    by_case = {}
    for (K, D, f64, max_rows, env), have in zip(SHAPES, answers[1]):
        shape, on, bufs = parent_workspace(K, D, f64, max_rows, env)
        head, _, plan = have.partition(" |")
        got = fields(head)
        for key, val in list(shape.items()) + list(on.items()):
            assert got[key] == val, (K, D, f64, max_rows, env, key, val, got[key])
        assert [tuple(b.split(":")) for b in plan.split()] == [(n, str(b), str(f)) for n, b, f in bufs], (K, D, f64, max_rows, env)
        counted = sum(b for _n, b, f in bufs if not f & PINNED)
        assert got["counted_bytes"] == counted
        by_case[K, D, f64, max_rows, tuple(env.items())] = (counted, correction(K, shape["npad"], shape["lists"]), bufs)
    # what the cases are there for
    assert by_case[1, 8, F32, 1000, ()][2][0][0] == "tri" and "xc" not in [b[0] for b in by_case[1, 8, F32, 1000, ()][2]]
    assert "xc" in [b[0] for b in by_case[1, 160, F32, 1000, ()][2]]
    assert not {"lists", "xp", "img_i8b"} & {b[0] for b in by_case[2, 64, F32, 2000000001, ()][2]}
    assert "img_i8b" not in [b[0] for b in by_case[6, 48, F32, 5000, ()][2]] and "img_i8b" in [b[0] for b in by_case[6, 49, F32, 5000, ()][2]]
    assert "lists" not in [b[0] for b in by_case[257, 64, F32, 2000, ()][2]]
    # the parent's own count on the GPU, corrected
    for key, parent in PARENT_BYTES.items():
        counted, corr, _bufs = by_case[key + ((),)]
        assert counted == parent + corr, (key, counted, parent, corr)
    for env, parent in zip(GPU_ENVS, PARENT_BYTES_ENV):
        counted, corr, _bufs = by_case[8, 64, F32, 5000, tuple(env.items())]
        assert counted == parent + corr, (env, counted, parent, corr)


def test_life_cycle_under_the_sanitizers(answers):
    """Every allocation failing in turn (alone and as a further tile), a group of three destroyed in all six orders, a tile
    larger than the first: the program checks live allocations, reference counts and the scratch itself and ends with ok=1;
    ASan, LeakSanitizer and UBSan had nothing to say (stderr is empty, the exit status 0)."""
    for (K, D, f64, max_rows), have in zip(GPU_SHAPES, answers[2]):
        _shape, _on, bufs = parent_workspace(K, D, f64, max_rows, {})
        got = fields(have)
        assert got["ok"] == 1 and got["allocations"] == len(bufs), (K, D, have)
        if D <= 256:
            assert got["tile_allocations"] == len([b for b in bufs if not b[2] & SCRATCH]), (K, D, have)
