"""MultilayerPerceptronClassifier at world sizes 1, 2 and 3 (gloo on CPU): the same global table and the same
``initialWeights`` fit to the same weights.

The rows are Double vectors, so every rank runs the fp64 host formulation and the world sizes differ in the order of
the fp64 sums only.  One evaluation sums 4000 rows: the loss and every gradient entry move by at most 4000 2^-53 =
4.4e-13 relative.  The fit makes 25 iterations, about 30 evaluations: 1.3e-11 if the perturbations only add up.
L-BFGS is not a contraction (a perturbed evaluation changes the curvature pairs and with them the later steps), so
the bound leaves two orders of magnitude for that: 1e-9 of the largest weight, the bound of the GaussianMixture test
as well (the gap measures 2e-14 .. 6e-14).  A shard dropped or counted twice changes every sum by 1 / 4000 and
fails it by five orders of magnitude.
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
    """test_distributed._run for the MLP worker."""
    out = tmp_path / f"mlp_{nproc}.json"
    env = dict(os.environ, CDNAML_DEVICE="cpu", OMP_NUM_THREADS="2", PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env["CDNAML_CONF_CDNAML__WAREHOUSE__DIR"] = str(tmp_path / f"wh{nproc}")
    worker = os.path.join(HERE, "mlp_dist_worker.py")
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


def test_same_weights_at_one_two_and_three_ranks(tmp_path):
    one = _run(tmp_path, 1)
    assert one["world"] == 1 and one["rows"] == [4000] and one["predicted"] == 4000
    assert one["iterations"] == 25 and one["objectiveHistory"][-1] < 0.9 * one["objectiveHistory"][0]
    w1 = np.array(one["weights"])
    for nproc in (2, 3):
        res = _run(tmp_path, nproc)
        assert res["world"] == nproc and sum(res["rows"]) == 4000 and res["predicted"] == 4000
        if nproc == 3:
            assert res["rows"][2] == 0 and min(res["rows"][:2]) > 0      # one empty shard
        assert res["iterations"] == one["iterations"]
        gap = np.abs(np.array(res["weights"]) - w1).max()
        print(f"mlp W = {nproc}: rows {res['rows']}, |weights - one rank's| = {gap:.2e} (largest weight "
              f"{np.abs(w1).max():.2f})")
        assert gap <= 1e-9 * np.abs(w1).max()
