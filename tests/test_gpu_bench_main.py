"""bench.py's main() on a small grid (``-m gpu``): a plain run reports the
headline fields alone, --full adds what it measures, --steps sets the timed
steps, and --dump-outputs reads the last timed step's rows before the --full
probe runs a sweep again. Both runs write the same files.

main() brings up torch's HIP runtime before the host library, so it runs in
a child process of its own (one for both runs), which logs every
bench.launch (a sweep's launches) and bench.dump_outputs call in order."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID, VARIANTS, STEPS, WARMUP = 10, 3, 2, 1
PLAIN = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
         "scaling", "vs_baseline", "dtype", "data", "config"}

CHILD = r"""
import contextlib, io, json, sys
sys.path.insert(0, sys.argv[1])
import bench

runs = json.loads(sys.argv[2])
events = []
dump = bench.dump_outputs
bench.dump_outputs = lambda *a: (events.append("dump"), dump(*a))[1]
launch = bench.launch
bench.launch = lambda sw: (events.append("run"), launch(sw))[1]
out = []
for argv in runs:
    del events[:]
    sys.argv = ["bench.py"] + argv
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        bench.main()
    out.append({"stdout": buf.getvalue(), "events": list(events)})
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    base = tmp_path_factory.mktemp("bench_main")
    a, b = str(base / "plain"), str(base / "full")
    common = ["--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--grid", str(GRID),
              "--topologies", str(VARIANTS)]
    argvs = [common + ["--dump-outputs", a],
             common + ["--dump-outputs", b, "--full", "--no-route-db", "--no-cpu-baseline", "--legs", ""]]
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps(argvs)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    for x in res:
        lines = x["stdout"].strip().splitlines()
        assert len(lines) == 1  # one result line
        x["line"] = json.loads(lines[0])
    return res[0], res[1], a, b


def test_plain_run_reports_the_headline_alone(runs):
    plain, _, _, _ = runs
    line = plain["line"]
    assert set(line) == PLAIN
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["ms_per_step"] > 0
    # value = sources swept per second of the timed steps; the line rounds
    # ms_per_step to 1e-4 ms (half a unit either way) and value to 0.1
    assert line["value"] == pytest.approx(VARIANTS * GRID * GRID / (line["ms_per_step"] * 1e-3),
                                          rel=6e-5 / line["ms_per_step"] + 1e-6, abs=0.1)
    # nothing runs after the timed steps but the dump
    assert plain["events"] == ["run"] * (VARIANTS * (WARMUP + STEPS)) + ["dump"]


def test_full_run_dumps_before_its_probe(runs):
    _, full, _, _ = runs
    assert set(full["line"]) == PLAIN | {"roofline"}
    timed = VARIANTS * (WARMUP + STEPS)
    events = full["events"]
    assert events[:timed + 1] == ["run"] * timed + ["dump"]
    assert len(events) > timed + 1 and set(events[timed + 1:]) == {"run"}  # the probe, after the dump


def test_both_runs_dump_the_same_rows(runs):
    _, _, a, b = runs
    files = sorted(os.listdir(a))
    assert files == sorted(f"{kind}_v{t:03d}.npy" for t in range(VARIANTS)
                           for kind in ("sources", "dist", "first_hops"))
    assert files == sorted(os.listdir(b))
    for f in files:
        assert np.array_equal(np.load(os.path.join(a, f)), np.load(os.path.join(b, f))), f
    # variant 0 is the undrained grid: unit metrics, Manhattan distances
    rr, cc = np.divmod(np.arange(GRID * GRID), GRID)
    dist = np.load(os.path.join(a, "dist_v000.npy"))
    for k, s in enumerate(np.load(os.path.join(a, "sources_v000.npy")).astype(int)):
        assert np.array_equal(dist[k], np.abs(rr - rr[s]) + np.abs(cc - cc[s]))
