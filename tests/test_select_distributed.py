"""The univariate tests and UnivariateFeatureSelector at world sizes 1, 2 and 3 (gloo on CPU) on the same global table.

The contingency tables, the degrees of freedom and the selected features are integers and must be identical at every
world size.  The ANOVA and F-value statistics are fp64 sums taken in another order (and about another shift) at every
world size, so they are not compared with each other: each meets the criterion of tests/_select_refs.py against the
longdouble reference (at most M = 8 times the error of the plain numpy fp64 yardstick, floor 4 fp64 ulps).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _select_refs as R
from tests.select_dist_worker import CC, D, KC, KEPT, tables
from tests.test_distributed import _free_port, _port_clash

pytestmark = pytest.mark.slow

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _run(tmp_path, nproc):
    """test_distributed._run for the selectors' worker."""
    out = tmp_path / f"select_{nproc}.json"
    env = dict(os.environ, CDNAML_DEVICE="cpu", OMP_NUM_THREADS="2", PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env["CDNAML_CONF_CDNAML__WAREHOUSE__DIR"] = str(tmp_path / f"wh{nproc}")
    worker = os.path.join(HERE, "select_dist_worker.py")
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


def test_same_tables_and_selection_at_one_two_and_three_ranks(tmp_path):
    Xk, Xc, codes, y = (a[:KEPT] for a in tables())
    table = R.count_table(Xk, codes, KC, CC)[0]
    shift, yshift = R.shift_of(Xc), float(np.mean(y[:1024]))
    ref_a, ref_f = R.anova_f_reference(Xc, codes), R.fvalue_f_reference(Xc, y)
    yard_a = R.anova_from_sums(*R.class_yardstick(Xc, codes, CC, shift))
    yard_f = R.fvalue_from_sums(*R.regress_yardstick(Xc, y, shift, yshift))
    one = None
    for nproc in (1, 2, 3):
        res = _run(tmp_path, nproc)
        assert res["world"] == nproc and sum(res["rows"]) == KEPT
        if nproc == 3:
            assert res["rows"][2] == 0 and min(res["rows"][:2]) > 0      # one empty shard
        assert np.array_equal(np.array(res["table"]).reshape(D, KC, CC), table)
        assert res["chi2"][1] == [R.chi2_reference(t)[1] for t in table]
        assert res["anova"][1] == [KEPT - 1] * D and res["fvalue"][1] == [KEPT - 2] * D
        R.check(f"W = {nproc} anova F", res["anova"][2], ref_a, yard_a)
        R.check(f"W = {nproc} F-value", res["fvalue"][2], ref_f, yard_f)
        if one is None:
            one = res
            assert all(len(v) == 3 for v in one["selected"].values())
        assert res["selected"] == one["selected"] and res["chi2"] == one["chi2"]
