"""AFTSurvivalRegression at world sizes 1, 2 and 3 (gloo on CPU): the same global table fits to the same parameters.

The rows are Double vectors, so every rank runs the fp64 host formulation and the world sizes differ in the order of
the fp64 sums only: every evaluation moves by ~n 2^-53 relative, and with tol = 1e-14 each fit runs to the optimum
of (nearly) the same function.  Two different optimisers (this one and scipy's L-BFGS-B) agree to ~1e-8 on such a
table (tests/test_aft_cpu.py), so the bound is 1e-6 of the largest parameter; a shard dropped or counted twice moves
the estimate by its statistical error, ~1e-2.
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
    """test_distributed._run for the AFT worker."""
    out = tmp_path / f"aft_{nproc}.json"
    env = dict(os.environ, CDNAML_DEVICE="cpu", OMP_NUM_THREADS="2", PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env["CDNAML_CONF_CDNAML__WAREHOUSE__DIR"] = str(tmp_path / f"wh{nproc}")
    worker = os.path.join(HERE, "aft_dist_worker.py")
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


def test_same_parameters_at_one_two_and_three_ranks(tmp_path):
    one = _run(tmp_path, 1)
    assert one["world"] == 1 and one["rows"] == [4000] and one["predicted"] == 4000
    t1 = np.array(one["theta"])
    assert abs(np.exp(t1[-1]) - 0.7) < 0.05          # the generating scale: the fit is a real one
    for nproc in (2, 3):
        res = _run(tmp_path, nproc)
        assert res["world"] == nproc and sum(res["rows"]) == 4000 and res["predicted"] == 4000
        if nproc == 3:
            assert res["rows"][2] == 0 and min(res["rows"][:2]) > 0      # one empty shard
        gap = np.abs(np.array(res["theta"]) - t1).max()
        print(f"aft W = {nproc}: rows {res['rows']}, |theta - one rank's| = {gap:.2e} (largest parameter "
              f"{np.abs(t1).max():.2f})")
        assert gap <= 1e-6 * np.abs(t1).max()
