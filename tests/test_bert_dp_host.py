"""Host side of bert_pretrain.py / finetune_bert.py on several GPUs (no GPU needed): how the rows of a global batch are dealt
(dist.deal_rows), the weights that make unequal shares average to the global mean (dist.loss_shares, two gloo ranks on the CPU in
the manner of tests/test_dp_gloo.py), and the usage error for a --batch_size the world size does not divide."""
import math
import os
import socket
import subprocess
import sys

import pytest
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = [(3, 1), (0, 5), (2, 2), (0, 0)]          # the labelled rows of rank 0 and rank 1, one exchange each


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("rows", [0, 1, 2, 3, 4, 7, 32])
def test_deal_rows_is_a_contiguous_ordered_even_cover(rows, world):
    from item_alignment_amd.dist import deal_rows
    slices = [deal_rows(rows, r, world) for r in range(world)]
    assert slices[0][0] == 0 and slices[-1][1] == rows
    assert all(a[1] == b[0] for a, b in zip(slices, slices[1:]))               # contiguous and in rank order
    sizes = [hi - lo for lo, hi in slices]
    assert all(n >= 0 for n in sizes) and max(sizes) - min(sizes) <= 1
    assert sizes == sorted(sizes, reverse=True) and sizes[:rows % world] == [rows // world + 1] * (rows % world)
    assert [i for lo, hi in slices for i in range(lo, hi)] == list(range(rows))


def test_loss_shares_without_a_process_group():
    from item_alignment_amd.dist import loss_shares
    weights, totals = loss_shares([5, 3])
    assert weights == [1.0, 1.0] and totals == [5, 3]
    weights, totals = loss_shares([0, 3])
    assert math.isnan(weights[0]) and weights[1] == 1.0 and totals == [0, 3]


def _worker(rank, world, port, out):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from item_alignment_amd import dist as iadist
    assert iadist.env_ranks() == (rank, world, rank)
    iadist.init_from_env("cpu")
    got = []
    for pair in COUNTS:
        # two terms in one exchange, as bert_pretrain.py sends them: the labelled rows, and a row count that is never 0
        weights, totals = iadist.loss_shares([pair[rank], rank + 1])
        got.append((weights, totals))
    out[rank] = got
    dist.destroy_process_group()


def test_loss_shares_over_two_gloo_ranks():
    world = 2
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    for i, pair in enumerate(COUNTS):
        (w0, t0), (w1, t1) = out[0][i], out[1][i]
        total = sum(pair)
        assert t0 == t1 == [total, 3]
        assert (w0[1], w1[1]) == (1 * 2 / 3, 2 * 2 / 3)
        if total == 0:                         # no labelled row on any rank: the mean over no row, NaN as in one process
            assert math.isnan(w0[0]) and math.isnan(w1[0])
            continue
        assert (w0[0], w1[0]) == (pair[0] * 2 / total, pair[1] * 2 / total)
        # what the reducer does with the ranks' terms: the mean.  The weights average to 1 ...
        assert abs((w0[0] + w1[0]) / world - 1.0) < 1e-15
        # ... and rank means m_r weighted so average to the mean over all rows: (n_0 m_0 + n_1 m_1) / N
        m = (0.25, 4.0)
        want = (pair[0] * m[0] + pair[1] * m[1]) / total
        assert abs((w0[0] * m[0] + w1[0] * m[1]) / world - want) < 1e-15
        assert (w0[0] == 0.0) == (pair[0] == 0) and (w1[0] == 0.0) == (pair[1] == 0)      # a rank without rows adds exactly 0


@pytest.mark.parametrize("script,more", [("bert_pretrain.py", []), ("finetune_bert.py", [])])
def test_a_batch_size_the_world_does_not_divide_is_a_usage_error(tmp_path, script, more):
    """before the GPU check, before the model directory is looked at, before anything is read or written"""
    out = tmp_path / "out"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    argv = ["--data_dir", str(tmp_path / "no_data"), "--model_name_or_path", str(tmp_path / "no_model"), "--output_dir", str(out),
            "--batch_size", "3"] + more
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv, capture_output=True, text=True, env=env, timeout=120, cwd=ROOT)
    assert r.returncode != 0
    assert "--batch_size 3 must be divisible by the world size 2" in r.stderr, r.stderr[-2000:]
    assert "usage:" in r.stderr
    assert not out.exists()
