"""`bench.py --dump-outputs DIR`: what the timed path computed in its last step, as .npy files of bounded size, on the same
points from run to run; and `--steps` is the number of timed steps."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_index_takes_every_point_that_fits_and_a_fixed_sample_otherwise(bench):
    assert np.array_equal(bench.dump_index(65_536, 8 * 13), np.arange(65_536))
    big = bench.dump_index(1_048_576, 8 * 13)
    assert big.size * 8 * 13 <= bench.DUMP_MAX_BYTES and big.size > 500_000
    assert np.all(np.diff(big) > 0) and big[-1] < 1_048_576
    assert np.array_equal(big, bench.dump_index(1_048_576, 8 * 13))


def test_dump_outputs_writes_float_arrays_and_refuses_more_than_the_limit(bench, tmp_path):
    a_end = np.array([[1 + 2j, 3 - 4j]], dtype=np.complex64)
    arrays = bench.record_arrays(a_end, np.array([5.0], np.float32), np.array([6.0], np.float32),
                                 np.array([-1], np.int64), np.arange(1))
    bench.dump_outputs(str(tmp_path / "out"), arrays)
    got = {n: np.load(tmp_path / "out" / (n + ".npy")) for n in arrays}
    assert got["a_end"].dtype == np.float32 and got["a_end"].tolist() == [[[1, 2], [3, -4]]]
    assert got["first_bad_step"].dtype == np.float64 and got["first_bad_step"].tolist() == [-1.0]
    assert got["index"].dtype == np.float64 and got["p_max"].dtype == np.float32
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "big"), {"x": np.zeros(bench.DUMP_MAX_BYTES // 8 + 1)})
    assert not (tmp_path / "big").exists()


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"]])
def test_steps_and_warmup_are_validated(bench, monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step(tmp_path, oracle):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--no-cpu-baseline", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["steps"] == 3
    d = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert sum(a.nbytes for a in d.values()) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    n = 65_536
    assert np.array_equal(d["index"], np.arange(n)) and d["a_end"].shape == (n, 4, 2)
    assert np.all(d["first_bad_step"] == -1) and d["n_finite"][0] == n
    assert d["best_index"][0] == np.argmax(d["gain"]) and d["best_gain"][0] == d["gain"].max()
    pick = np.array([1, n // 5, n - 2])
    ref = oracle.sweep(np.linspace(-0.05, 0.05, n)[pick], z_max=1000.0, n=100_000, save_every=10, gamma=0.0115,
                       alpha=1.15e-4, a0=np.sqrt([0.5, 0.5, 1e-5, 1e-5]).astype(complex), threads=3)
    got = d["a_end"][pick, :, 0] + 1j * d["a_end"][pick, :, 1]
    assert np.max(np.abs(got - ref["a_end"]) / np.abs(ref["a_end"])) < 1e-9
