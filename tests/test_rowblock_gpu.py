"""The row split that K24 to K27 share (``split_rows`` of csrc/kernels/rowblock.h), through the four plan functions,
at the sizes where a rounding slip would show.  The plan calls launch nothing and X is never filled, so every case
takes milliseconds.
"""
import pytest
import torch

from cdnaml.ops import kernels as K

pytestmark = pytest.mark.gpu

ROWS = 64  # the tile


def split(n, cap):
    """n rows over at most ``cap`` blocks of at least 1024 rows, a multiple of the tile per block, every block with
    rows: the formula, restated."""
    nb = max(1, min(-(-n // 1024), cap))
    rpb = -(-(-(-n // nb)) // ROWS) * ROWS
    return -(-n // rpb), rpb


def sizes(cap):
    return [1, 63, 64, 65, 1023, 1024, 1025, 65 * 1024, cap * 1024, cap * 1024 + 1]


# (name, cap, d, the plan of X)
CASES = [
    ("mlp", 1024, 4, lambda X: K.mlp_plan(X, [4, 3])),
    ("fm", 768, 4, lambda X: K.fm_plan(X, 2)),
    ("fm two-slot", 512, 65, lambda X: K.fm_plan(X, 32)),   # more than four gradient tiles: two blocks per CU
    ("aft", 768, 4, lambda X: K.aft_plan(X)),
    ("label regress", 4 * 256, 4, lambda X: K.label_stats_plan(X, K.LABEL_REGRESS)),
    ("label class", 4 * 256, 4, lambda X: K.label_stats_plan(X, K.LABEL_CLASS, C=2)),
    ("label count", 4 * 256, 4, lambda X: K.label_stats_plan(X, K.LABEL_COUNT, C=2, K=2)),
    ("label count, wide table", 1 * 256, 4, lambda X: K.label_stats_plan(X, K.LABEL_COUNT, C=64, K=64)),
]


@pytest.mark.parametrize("name,cap,d,plan_of", CASES, ids=[c[0] for c in CASES])
def test_split(name, cap, d, plan_of, gpu_device):
    base = torch.empty((cap * 1024 + 1, d), dtype=torch.float32, device=gpu_device)  # never filled
    for n in sizes(cap):
        pl = plan_of(base[:n])
        assert pl["path"] == "native", (name, n)
        if "blocks_per_cu" in pl:
            assert pl["blocks_per_cu"] * 256 == cap, (name, n, pl)
        nblk, rpb = pl["nblk"], pl["rows_per_block"]
        assert (nblk, rpb) == split(n, cap), (name, n, pl)
        assert rpb % ROWS == 0, (name, n, pl)
        assert (nblk - 1) * rpb < n <= nblk * rpb, (name, n, pl)
        assert nblk <= cap, (name, n, pl)
