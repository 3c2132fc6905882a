"""The ONE JSON line bench.py prints is what the driver records: its keys (the contract's, `roofline` with both fractions,
`cpu_baseline`, the sub-lines) and its size (< 6 KB: round 4's 22-KB line did not parse in the driver's record) are pinned here
on a full record of a real run (profiles/r6_bench_detail_sample.json, made on the GPU by `bench.py --full --detail`), without a GPU."""
import json
import os

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _record():
    with open(os.path.join(ROOT, "profiles", "r6_bench_detail_sample.json")) as f:
        return json.load(f)


def test_compact_line_has_the_contracts_keys_and_fits():
    out = _record()
    line = bench.compact_line(out)
    text = json.dumps(line)
    assert len(text) < 6000, len(text)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in line, key
    assert line["metric"].startswith("GMM-VB E+M samples/sec at K=64,D=128,N=1e7") and line["unit"] == "samples/s"
    assert line["vs_baseline"] is None and line["dtype"] == "f64" and line["data"] == "synthetic" and line["higher_is_better"] is True
    assert "workload" in line["config"] and "model" not in line["config"]
    r = line["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic", "frac_executed", "frac_on_F", "step_frac_on_F", "pruned"):
        assert key in r, key
    assert r["bound"] in ("hbm", "mfma") and 0.0 < r["frac"] <= 1.0 and r["frac"] == r["frac_executed"]
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert r["pruned"] is True and r["frac_on_F"] > 1.0            # the F-basis fraction of a pruned pass is not a utilisation
    c = line["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and "threads_swept" in c
    for sub in ("hmm_c5", "c2", "c4_shard", "c4_strong"):
        assert sub in line, sub
    for sub in ("c2", "c4_shard", "c4_strong"):
        for key in ("ms_per_step", "kernel", "frac_executed", "frac_on_F", "workload"):
            assert key in line[sub], (sub, key)
    assert line["parity"]["passed"] and line["parity_sparse_path"]["passed"]
    assert line["parity"]["max_rel_err"] < 1e-5 and line["parity"]["tolerance"] == 1e-5


def test_value_is_rows_over_time():
    out = _record()
    assert abs(out["value"] - out["config"]["rows_total"] / (out["ms_per_step"] * 1e-3)) < 1e-6 * out["value"]


def test_plain_line_has_the_contracts_keys():
    """A run without --full: no roofline, cpu_baseline, parity or legs in the record; the line keeps the contract's keys."""
    out = _record()
    for k in ("roofline", "cpu_baseline", "parity", "parity_sparse_path", "dense", "full_fit", "hmm_c5", "c2", "c4_shard",
              "c4_strong", "hard_workload", "spread_sweep", "offpath"):
        out[k] = None
    out["per_step"] = {"wall_ms": out["per_step"]["wall_ms"]}
    line = bench.compact_line(out)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "window"):
        assert key in line, key
    assert "roofline" not in line and "cpu_baseline" not in line and "parity" not in line
    assert line["steps"] == out["steps"] and line["ms_per_step"] == out["ms_per_step"]


class _FakeEngine:
    """Responsibilities read-out whose row i holds i + k / K: the rows read can be told from their values."""

    def __init__(self, K, n):
        self.K, self.n = K, n

    def responsibilities(self, row0, n_rows):
        import torch
        assert 0 <= row0 and n_rows >= 1 and row0 + n_rows <= self.n, (row0, n_rows, self.n)
        return torch.arange(row0, row0 + n_rows, dtype=torch.float64)[:, None] + torch.arange(self.K, dtype=torch.float64) / self.K


class _FakeWorkload:
    """What dump_outputs reads of a bench.Workload: the K-side state (posterior, statistics), the lower bound, the engine."""

    def __init__(self, K, D, n):
        import torch
        from types import SimpleNamespace
        g = torch.Generator().manual_seed(K * 1000 + D)

        def rand(*shape):
            return torch.rand(*shape, generator=g, dtype=torch.float64)

        q = SimpleNamespace(alpha=rand(K), m=rand(K, D), kappa=rand(K), nu=rand(K), w=rand(K, D, D), w_inv=rand(K, D, D))
        self.ks = SimpleNamespace(q=q, ns=rand(K), x_bar=rand(K, D), s=rand(K, D, D))
        self.K, self.D, self.n = K, D, n
        self.terms = {"vl": -1234.5}
        self.eng = _FakeEngine(K, n)


def _dump(tmp_path, name, K, D, n):
    d = tmp_path / name
    w = _FakeWorkload(K, D, n)
    bench.dump_outputs(str(d), w)
    return w, {p.stem: np.load(p) for p in d.iterdir()}


def test_dump_outputs_writes_what_the_caller_receives(tmp_path):
    K, D, n = 64, 128, 10_000_000
    w, got = _dump(tmp_path, "a", K, D, n)
    assert set(got) == {"hn_alpha_vec", "hn_m_vecs", "hn_kappas", "hn_nus", "hn_w_mats", "hn_w_mats_inv", "ns", "x_bar_vecs",
                        "s_mats", "vl", "r_vecs"}
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(os.path.getsize(p) for p in (tmp_path / "a").iterdir()) <= 64_000_000
    np.testing.assert_array_equal(got["hn_w_mats"], w.ks.q.w.numpy())
    np.testing.assert_array_equal(got["s_mats"], w.ks.s.numpy())
    assert got["vl"].tolist() == [-1234.5]
    r = got["r_vecs"]
    assert r.shape[1] == K and r.shape[0] >= 16 * 1024
    idx = r[:, 0]
    assert np.all(np.diff(idx) > 0) and np.all(idx == np.floor(idx)) and idx[-1] < n      # whole rows, in row order, in range
    np.testing.assert_array_equal(r - idx[:, None], np.broadcast_to(np.arange(K) / K, r.shape))
    _, again = _dump(tmp_path, "b", K, D, n)                  # a fixed sample: the same rows every run
    for k in got:
        np.testing.assert_array_equal(got[k], again[k])


def test_dump_outputs_stays_within_64_mb_at_any_size(tmp_path):
    for K, D, n in ((512, 256, 3000), (8, 2, 100), (300, 64, 1_000_000)):
        _, got = _dump(tmp_path, f"k{K}d{D}", K, D, n)
        assert sum(os.path.getsize(p) for p in (tmp_path / f"k{K}d{D}").iterdir()) <= 64_000_000
        assert got["r_vecs"].shape[1] == K and 1 <= got["r_vecs"].shape[0] <= n
        assert got["hn_w_mats"].shape[1:] == (D, D) and got["hn_w_mats"].shape[0] == got["ns"].shape[0] >= 1
