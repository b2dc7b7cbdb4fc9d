"""FMRegressor (adamW) and FMClassifier (gd) at world sizes 1, 2 and 3 (gloo on CPU): the same global table, seed and
``miniBatchFraction = 0.5`` fit to the same parameters.

The minibatch is drawn by a Philox keyed by the global row id, so every world size selects the same rows: the
selected count of every iteration must be identical, which a selection keyed by the local row would fail at once.
The rows are Double vectors, so every rank runs the fp64 host formulation and the world sizes differ in the order of
the fp64 sums only.  One step sums about 2000 rows: the loss and every gradient entry move by at most 2000 2^-53 =
2.2e-13 relative; 25 iterations: 6e-12 if the perturbations only add up.  AdamW divides by sqrt(v-hat), which
amplifies a perturbation of a small gradient entry, so the bound leaves two orders of magnitude: 1e-9 of the largest
parameter, the bound and the argument of tests/test_mlp_distributed.py.  A shard dropped or counted twice changes
every sum by 1 / 4000 and fails it by five orders of magnitude.
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
    """test_distributed._run for the FM worker."""
    out = tmp_path / f"fm_{nproc}.json"
    env = dict(os.environ, CDNAML_DEVICE="cpu", OMP_NUM_THREADS="2", PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env["CDNAML_CONF_CDNAML__WAREHOUSE__DIR"] = str(tmp_path / f"wh{nproc}")
    worker = os.path.join(HERE, "fm_dist_worker.py")
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
    assert one["world"] == 1 and one["rows"] == [4000]
    for name in ("regressor", "classifier"):
        m = one[name]
        assert m["predicted"] == 4000 and len(m["counts"]) == 25 and m["loss"][-1] < 0.9 * m["loss"][0]
        assert all(1800 < c < 2200 for c in m["counts"]) and len(set(m["counts"])) > 5   # a fresh draw per iteration
    for nproc in (2, 3):
        res = _run(tmp_path, nproc)
        assert res["world"] == nproc and sum(res["rows"]) == 4000
        if nproc == 3:
            assert res["rows"][2] == 0 and min(res["rows"][:2]) > 0      # one empty shard
        for name in ("regressor", "classifier"):
            assert res[name]["predicted"] == 4000
            assert res[name]["counts"] == one[name]["counts"]
            t1 = np.array(one[name]["theta"])
            gap = np.abs(np.array(res[name]["theta"]) - t1).max()
            print(f"fm {name} W = {nproc}: rows {res['rows']}, |theta - one rank's| = {gap:.2e} (largest "
                  f"parameter {np.abs(t1).max():.2f})")
            assert gap <= 1e-9 * np.abs(t1).max()
