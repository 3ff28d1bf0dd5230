"""bench.py without a GPU: the options, the plain result line's fields, and
--dump-outputs' seeded sample of the sweeps' rows over stand-in sweeps
(tests/test_gpu_bench_main.py runs main() itself)."""
import os
import types

import numpy as np
import pytest

import bench


class FakeSweep:
    """fetch(i) as SpfSweep returns it: u32 dist[N], u32 first hops[N * W],
    nodes in the link state's id order."""

    def __init__(self, nodes, words, salt):
        self.nodes, self.words, self.salt = nodes, words, salt

    def fetch(self, i):
        dist = (np.arange(self.nodes, dtype=np.uint32) * 7 + i + self.salt)
        dist[-1] = 0xFFFFFFFF  # unreachable marker survives the float64 copy
        nh = np.arange(self.nodes * self.words, dtype=np.uint32) + 1000 * i
        return dist, nh


def _sweeps(nodes, words, variants):
    names = [str(v) for v in reversed(range(nodes))]  # id order != name order
    ls = types.SimpleNamespace(_impl=types.SimpleNamespace(node_names=lambda: names))
    srcs = [str(v) for v in range(nodes)]
    out = [(t, srcs, ls, FakeSweep(nodes, words, t)) for t in range(variants)]
    return out + [(variants, [], ls, None)], names


def test_dump_outputs_rows_in_name_order_and_repeatable(tmp_path):
    sweeps, names = _sweeps(37, 2, 3)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, sweeps, 0, 1)
    bench.dump_outputs(b, sweeps, 0, 1)
    files = sorted(os.listdir(a))
    assert files == sorted(f"{kind}_v{t:03d}.npy" for t in range(3)
                           for kind in ("sources", "dist", "first_hops"))
    assert files == sorted(os.listdir(b))
    for f in files:
        x = np.load(os.path.join(a, f))
        assert x.dtype == np.float64
        assert np.array_equal(x, np.load(os.path.join(b, f)))
    ids = {name: i for i, name in enumerate(names)}
    order = np.array([ids[str(v)] for v in range(37)])
    for t, srcs, _, sw in sweeps[:3]:
        picked = np.load(os.path.join(a, f"sources_v{t:03d}.npy")).astype(int)
        dist = np.load(os.path.join(a, f"dist_v{t:03d}.npy"))
        hops = np.load(os.path.join(a, f"first_hops_v{t:03d}.npy"))
        assert dist.shape == (len(picked), 37) and hops.shape == (len(picked), 37, 2)
        for k, s in enumerate(picked):
            d, nh = sw.fetch(srcs.index(str(s)))
            assert np.array_equal(dist[k], d[order].astype(np.float64))
            assert np.array_equal(hops[k], nh.reshape(37, 2)[order].astype(np.float64))
        assert dist.max() == float(0xFFFFFFFF)


def _array_bytes(out):
    return sum(np.load(os.path.join(out, f)).nbytes for f in os.listdir(out))


def test_dump_outputs_samples_nodes_when_a_row_does_not_fit(tmp_path, monkeypatch):
    """8 sweeps share 4 KiB: 512 B each against a 3.2 KB row, so each keeps
    one source and (512 - 8) // (8 * 3) = 21 of its 200 nodes."""
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 12)
    sweeps, names = _sweeps(200, 1, 8)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, sweeps, 0, 1)
    bench.dump_outputs(b, sweeps, 0, 1)
    assert 0 < _array_bytes(a) <= 1 << 12
    assert len(os.listdir(a)) == 4 * 8
    ids = {name: i for i, name in enumerate(names)}
    order = np.array([ids[str(v)] for v in range(200)])
    for t, srcs, _, sw in sweeps[:8]:
        nodes = np.load(os.path.join(a, f"nodes_v{t:03d}.npy"))
        assert nodes.dtype == np.float64 and len(nodes) == 21 and np.all(np.diff(nodes) > 0)
        assert np.array_equal(nodes, np.load(os.path.join(b, f"nodes_v{t:03d}.npy")))
        picked = np.load(os.path.join(a, f"sources_v{t:03d}.npy")).astype(int)
        assert len(picked) == 1
        d, nh = sw.fetch(srcs.index(str(picked[0])))
        sel = order[nodes.astype(int)]
        assert np.array_equal(np.load(os.path.join(a, f"dist_v{t:03d}.npy")), d[sel][None].astype(np.float64))
        assert np.array_equal(np.load(os.path.join(a, f"first_hops_v{t:03d}.npy")),
                              nh.reshape(200, 1)[sel][None].astype(np.float64))


def test_dump_outputs_writes_fewer_sweeps_when_not_all_fit(tmp_path, monkeypatch):
    """100 bytes hold the smallest dump (8 * (3 + W) = 32 B) of 3 sweeps, not of 8."""
    monkeypatch.setattr(bench, "DUMP_BYTES", 100)
    sweeps, _ = _sweeps(200, 1, 8)
    out = str(tmp_path / "o")
    bench.dump_outputs(out, sweeps, 0, 1)
    assert 0 < _array_bytes(out) <= 100
    assert sorted(f for f in os.listdir(out) if f.startswith("dist")) == [f"dist_v{t:03d}.npy" for t in range(3)]


def test_steps_must_be_positive(monkeypatch, capsys):
    for bad in ("0", "-3"):
        monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", bad, "--warmup", "1"])
        with pytest.raises(SystemExit) as e:
            bench.parse()
        assert e.value.code == 2
        assert "--steps" in capsys.readouterr().err


def test_plain_options_and_result_line(monkeypatch):
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    args = bench.parse()
    assert (args.steps, args.warmup, args.full, args.dump_outputs) == (7, 2, False, None)
    line = bench.result_line(args, 1, 1.25e7, 25.6, 10000, 39600, 320000)
    assert set(line) == {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                         "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"}
    assert (line["value"], line["unit"], line["ms_per_step"], line["steps"]) == (1.25e7, "SPF-sources/s", 25.6, 7)
    assert line["higher_is_better"] is True and line["dtype"] == "u32"
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--dump-outputs", "d"])
    args = bench.parse()
    assert args.full and args.dump_outputs == "d"


def test_dump_outputs_stays_under_the_size_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 16)
    sweeps, _ = _sweeps(200, 1, 8)  # all rows: 8 * 200 * 200 * 2 * 8 B = 5 MB
    for world in (1, 2):
        out = str(tmp_path / f"w{world}")
        for rank in range(world):
            bench.dump_outputs(out, sweeps, rank, world)
        rows = sum(np.load(os.path.join(out, f)).nbytes for f in os.listdir(out)
                   if not f.startswith("sources"))
        assert 0 < rows <= 1 << 16
        assert all(("_r" in f) == (world > 1) for f in os.listdir(out))
