"""bench.py's options without a GPU: a plain run times the PDQ phase alone (the other legs need --full), and --dump-outputs writes the
hashes exactly, as float32, within its size cap (a seeded sample of rows beyond it, with the row numbers beside them)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


@pytest.mark.parametrize("argv,msg", [(["--only", "hamming"], "needs --full"), (["--only", "pdq,jpeg"], "needs --full"),
                                      (["--full", "--only", "hamming_1m"], "unknown phase"), (["--steps", "0"], "at least 1"),
                                      (["--full", "--only", "e2e", "--dump-outputs", "out"], "must include pdq")])
def test_bench_rejects_before_touching_the_gpu(argv, msg):
    r = subprocess.run([sys.executable, BENCH] + argv, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and msg in r.stderr, r.stderr


def _bench_module():
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_exact_and_capped(tmp_path):
    import torch

    bench = _bench_module()
    h = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (5000, 32), dtype=np.uint8))
    bench.dump_outputs(str(tmp_path / "all"), h, 0, 1, np)
    got = np.load(tmp_path / "all" / "pdq_hash.npy")
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.uint8), h.numpy())
    assert sorted(os.listdir(tmp_path / "all")) == ["pdq_hash.npy"]

    bench.DUMP_BYTES = 2 * 1000 * (32 * 4 + 8)  # room for 1000 rows per rank at world 2
    samples = []
    for run in ("a", "b"):  # the sample is the same from run to run
        bench.dump_outputs(str(tmp_path / run), h, 1, 2, np)
        rows = np.load(tmp_path / run / "pdq_hash_rows_rank1.npy")
        got = np.load(tmp_path / run / "pdq_hash_rank1.npy")
        assert rows.dtype == np.float64 and len(rows) == 1000 and np.all(np.diff(rows) > 0)
        assert np.array_equal(got.astype(np.uint8), h.numpy()[rows.astype(np.int64)])
        samples.append(rows)
    assert np.array_equal(samples[0], samples[1])
