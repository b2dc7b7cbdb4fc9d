"""K.col_quantiles, RobustScaler and MaxAbsScaler at world sizes 1, 2 and 3 (gloo on CPU) on the same global table.

The per-rank digit tables are integers and all-reduce exactly, so the quantiles, the counts, the extrema and the fitted
model vectors must be bit-identical at every world size and equal to the numpy reference, for Float and for Double
vectors.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _quantile_refs as R
from tests.quantile_dist_worker import KEPT, LOWER, PROBS, UPPER, table
from tests.test_distributed import _free_port, _port_clash

pytestmark = pytest.mark.slow

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _run(tmp_path, nproc):
    """test_distributed._run for the quantiles' worker."""
    out = tmp_path / f"quantile_{nproc}.json"
    env = dict(os.environ, CDNAML_DEVICE="cpu", OMP_NUM_THREADS="2", PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env["CDNAML_CONF_CDNAML__WAREHOUSE__DIR"] = str(tmp_path / f"wh{nproc}")
    worker = os.path.join(HERE, "quantile_dist_worker.py")
    if nproc == 1:
        cmd = [sys.executable, worker, str(out)]
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), worker, str(out)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    if r.returncode != 0 and nproc > 1 and _port_clash(r.stderr):
        cmd[cmd.index("--master-port") + 1] = str(_free_port())
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads(out.read_text())


def expected(X):
    ref = R.quantiles(X, PROBS)
    med, rng = R.robust_reference(X, LOWER, UPPER)
    return {"dtype": "torch." + str(X.dtype), "q": R.bits(ref["q"]).reshape(-1).tolist(),
            "min": R.bits(ref["min"]).tolist(), "max": R.bits(ref["max"]).tolist(), "count": ref["count"].tolist(),
            "nan": ref["nan"].tolist(), "median": R.bits(med).tolist(), "range": R.bits(rng).tolist(),
            "maxAbs": R.bits(R.max_abs_reference(X)).tolist()}


def test_same_quantiles_and_scalers_at_one_two_and_three_ranks(tmp_path):
    X = table()[:KEPT]
    want = {"fp32": expected(X), "auto": expected(X.astype(np.float64))}
    for nproc in (1, 2, 3):
        res = _run(tmp_path, nproc)
        assert res["world"] == nproc and sum(res["rows"]) == KEPT
        if nproc == 3:
            assert res["rows"][2] == 0 and min(res["rows"][:2]) > 0      # one empty shard
        for precision in ("fp32", "auto"):
            assert res[precision] == want[precision], (nproc, precision)
