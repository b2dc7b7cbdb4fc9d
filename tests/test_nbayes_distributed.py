"""A 2-rank gloo NaiveBayes fit equals the 1-rank model: the count models to the bit (their sums are exact integers
whatever the sharding), the Gaussian one to rounding (the shift and the order of the partial sums differ)."""
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
    """test_distributed._run for the NaiveBayes worker."""
    out = tmp_path / f"nb_{nproc}.json"
    env = dict(os.environ, CDNAML_DEVICE="cpu", OMP_NUM_THREADS="2", PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env["CDNAML_CONF_CDNAML__WAREHOUSE__DIR"] = str(tmp_path / f"wh{nproc}")
    worker = os.path.join(HERE, "nbayes_dist_worker.py")
    cmd = [sys.executable, worker, str(out)] if nproc == 1 else \
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
         "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), worker, str(out)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    if r.returncode != 0 and nproc > 1 and _port_clash(r.stderr):
        cmd[cmd.index("--master-port") + 1] = str(_free_port())
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads(out.read_text())


def test_two_ranks_fit_the_one_rank_model(tmp_path):
    one, two = _run(tmp_path, 1), _run(tmp_path, 2)
    assert (one["world"], two["world"]) == (1, 2)
    for mt in ("multinomial", "complement", "bernoulli"):
        assert one[mt] == two[mt], mt
    for a, b in zip(one["gaussian"], two["gaussian"]):
        assert np.shape(a) == np.shape(b) and np.abs(np.asarray(a) / np.asarray(b) - 1).max() <= 1e-12
