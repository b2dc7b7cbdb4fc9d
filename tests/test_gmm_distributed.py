"""GaussianMixture at world sizes 1, 2 and 3 (gloo on CPU): the same global table fits to the same model.

The rows are Double vectors, so every rank runs the fp64 host formulation and the world sizes differ in the order of
the fp64 sums only: the same number of iterations, log-likelihood and parameters to relative 1e-9.  6001 rows: the
shards are uneven at W = 2 and W = 3.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_distributed import _free_port, _port_clash

pytestmark = pytest.mark.slow

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _run(tmp_path, nproc):
    """test_distributed._run for the GMM worker."""
    out = tmp_path / f"gmm_{nproc}.json"
    env = dict(os.environ, CDNAML_DEVICE="cpu", OMP_NUM_THREADS="2", PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env["CDNAML_CONF_CDNAML__WAREHOUSE__DIR"] = str(tmp_path / f"wh{nproc}")
    worker = os.path.join(HERE, "gmm_dist_worker.py")
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


def test_same_model_at_one_two_and_three_ranks(tmp_path):
    one = _run(tmp_path, 1)
    assert one["world"] == 1 and 2 < one["numIter"] < 100 and one["predicted"] == 6001
    for nproc in (2, 3):
        res = _run(tmp_path, nproc)
        assert res["world"] == nproc and res["predicted"] == 6001
        assert res["numIter"] == one["numIter"]
        assert res["clusterSizes"] == one["clusterSizes"] and sum(res["clusterSizes"]) == 6001
        assert abs(res["logLikelihood"] - one["logLikelihood"]) <= 1e-9 * abs(one["logLikelihood"])
        for name in ("weights", "means", "covs"):
            a, b = np.array(res[name]), np.array(one[name])
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-9 * np.abs(b).max(), err_msg=name)
